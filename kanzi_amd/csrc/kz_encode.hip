// kz_encode.hip -- the batched encoder: the codec span of EncodingTask.encodeBlock behind Sequence.forward, and the block-header kernels
#include "kz_pipe.h"

struct FrameEnc {
  int32_t* postLen;      // = batch d_len after the chain
  int32_t* skipFlags;    // [B]
  int32_t* hdrBytes;     // [B]
  int32_t* isCopy;       // [B] small block (<= 15 bytes): raw copy block
  int32_t* fallback;     // [B]
  int64_t* bits;         // [B] entropy payload bits -> final W
  u64* hash;             // [B] block checksum (XXHash32/64 of the original block)
  int chk;               // 0 none, 1 = 32 bit, 2 = 64 bit
  int nbFunctions;
};

// before entropy: header size per block (CompressedOutputStream.java:825-826, :861-896)
__global__ void k_frame_prepare(FrameEnc F, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int postLen = F.postLen[b];
  const int dataSize = (postLen < 256) ? 1 : (kz_ilog2((u32)postLen) >> 3) + 1;
  const bool two = !F.isCopy[b] && F.nbFunctions > 4;
  F.hdrBytes[b] = 1 + (two ? 1 : 0) + dataSize + 1 + (F.chk == 1 ? 4 : (F.chk == 2 ? 8 : 0));
}
// after entropy: decide the raw "transformed copy" fallback (:926-973)
__global__ void k_frame_decide(FrameEnc F, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t written = 8LL * F.hdrBytes[b] + F.bits[b];
  const int64_t entropyBytes = (written + 7) >> 3;
  F.fallback[b] = (!F.isCopy[b] && (int64_t)F.postLen[b] < entropyBytes) ? 1 : 0;
}
__global__ void k_frame_header(FrameEnc F, u8* __restrict__ out, int64_t outStride, kz_block_result* __restrict__ res, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  u8* o = out + (int64_t)b * outStride;
  const int postLen = F.postLen[b];
  const u32 skipFlags = (u32)F.skipFlags[b] & 0xFF;
  const int nb = F.nbFunctions;
  const int dataSize = (postLen < 256) ? 1 : (kz_ilog2((u32)postLen) >> 3) + 1;
  u32 mode = F.isCopy[b] ? 0x80u : 0u;
  mode |= (u32)(((dataSize - 1) & 3) << 5);
  u32 hsf = skipFlags;
  int idx = 0;
  int64_t written;
  if (postLen == 0) { res[b].bits = 0; res[b].length = 0; res[b].status = 0; res[b].skipFlags = 0xFF; res[b].mode = 0; return; }
  if (F.fallback[b]) {
    const u32 copyMode = (mode | (nb <= 4 ? (skipFlags >> 4) : 0x10u)) | 0x80u | 0x10u;     // :933-934
    o[idx++] = (u8)copyMode;
    if (nb > 4) { o[idx++] = (u8)skipFlags; hsf = skipFlags; } else hsf = ((copyMode << 4) | 0x0F) & 0xFF;
    mode = copyMode;
    written = 8LL * (F.hdrBytes[b] + postLen);
  } else {
    if ((mode & 0x80) || nb <= 4) {
      mode |= (skipFlags >> 4);
      hsf = (mode & 0x80) ? 0u : (((mode << 4) | 0x0F) & 0xFF);
      o[idx++] = (u8)mode;
    } else {
      mode |= 0x10;
      o[idx++] = (u8)mode; o[idx++] = (u8)skipFlags;
    }
    written = 8LL * F.hdrBytes[b] + F.bits[b];
  }
  for (int k = dataSize - 1; k >= 0; k--) o[idx++] = (u8)((u32)postLen >> (8 * k));
  o[idx++] = kz_block_cksum(mode & 0xFF, hsf, (u32)postLen, (u64)written);
  if (F.chk) {                                               // CompressedOutputStream.java:887-891
    const int nby = (F.chk == 1) ? 4 : 8;
    const u64 hv = F.hash[b];
    for (int k = nby - 1; k >= 0; k--) o[idx++] = (u8)(hv >> (8 * k));
  }
  res[b].bits = written; res[b].length = postLen; res[b].status = 0;
  res[b].skipFlags = (u8)skipFlags; res[b].mode = (u8)mode;
}

static bool frame_enc_alloc(kz_ctx* ctx, int B, int nbFunctions, FrameEnc& F) {
  F.skipFlags = kz_arena_array<int32_t>(ctx, B); F.hdrBytes = kz_arena_array<int32_t>(ctx, B);
  F.isCopy = kz_arena_array<int32_t>(ctx, B); F.fallback = kz_arena_array<int32_t>(ctx, B);
  F.bits = kz_arena_array<int64_t>(ctx, B); F.hash = kz_arena_array<u64>(ctx, B);
  F.chk = ctx->checksum; F.nbFunctions = nbFunctions;
  return F.skipFlags && F.hdrBytes && F.isCopy && F.fallback && F.bits && F.hash;
}

// =================================================================================================
// encode
// One call as the drivers see it.  blockSize = the stream's "blockSize" entry as TEXT reads it, fixed when the call was made (a
// queued job keeps the value of its submit time: later kz_ctx_set_block_size calls or kz_compress's scope do not reach it).
// pre (optional): the host stages' results for exactly these blocks, computed ahead (host_prestage) by the caller.
struct EncodePlan {
  uint64_t transformType; uint32_t entropyType; int32_t blockSize;
  const uint8_t* in; int64_t inStride; const int32_t* lengths; int B;
  uint8_t* out; int64_t outStride; kz_block_result* results; int32_t memKind; const HostPre* pre;
  Chain C; int maxN, maxLen;                        // encode_plan: the chain, the longest block, the longest a block gets in the chain
  bool host, textFwdGpu;                            // host memory; the TEXT stage runs on the device
};
// the chain and the layout contract of include/kanzi_hip.h, checked on the WHOLE batch before anything is copied or launched (a batch
// that is split would otherwise code its first part before a later part is refused)
static int encode_plan(kz_ctx* ctx, EncodePlan& p) {
  const int rc = chain_parse(ctx, p.transformType, p.entropyType, p.C);
  if (rc) return rc;
  p.maxN = 0;
  for (int b = 0; b < p.B; b++) { if (p.lengths[b] < 0) return -KZ_ERR_INVALID_PARAM; p.maxN = std::max(p.maxN, p.lengths[b]); }
  const int64_t needOut = kz_max_block_stream_bytes(p.maxN);
  if ((!p.in && p.maxN > 0) || !p.out || !p.results) { snprintf(ctx->err, sizeof(ctx->err), "encode: null pointer"); return -KZ_ERR_INVALID_PARAM; }
  if (p.outStride < needOut || (p.outStride & 3)) { snprintf(ctx->err, sizeof(ctx->err), "outStride %lld < %lld or not a multiple of 4", (long long)p.outStride, (long long)needOut); return -KZ_ERR_INVALID_PARAM; }
  // device output is written in place with 32-bit read-modify-write words (the bit concatenation of the entropy coders)
  if (p.memKind == KZ_MEM_DEVICE && ((uintptr_t)p.out & 3)) { snprintf(ctx->err, sizeof(ctx->err), "device out %p is not 4-byte aligned", (void*)p.out); return -KZ_ERR_INVALID_PARAM; }
  if (p.B > 1 && p.inStride < (int64_t)p.maxN) { snprintf(ctx->err, sizeof(ctx->err), "inStride %lld < longest block %d", (long long)p.inStride, p.maxN); return -KZ_ERR_INVALID_PARAM; }
  p.maxLen = seq_max_len(p.C.types, p.C.nb, p.maxN);
  // blocks go up to the reference's 1 GiB (BWT.java:59); BWT / RANK / MTFT blocks of 2^24 bytes and more take the wide forms of the
  // inverse kernels (8-byte links in kz_bwt_inv.hip, the plain list in kz_sbrt.hip: round 5), slower but the same bytes
  if (p.maxLen > KZ_MAX_BLOCK) { snprintf(ctx->err, sizeof(ctx->err), "block of %d bytes: blocks go up to %d bytes", p.maxN, KZ_MAX_BLOCK - 1057); return -KZ_ERR_BLOCK_SIZE; }
  p.host = p.memKind == KZ_MEM_HOST;
  p.textFwdGpu = !p.pre && kz_text_fwd_gpu_applies(ctx, p.transformType, p.entropyType, p.B);   // ONE predicate (kz_stream.hip asks the same one)
  return 0;
}
// blocks [b0, b0 + cnt) as a call of their own (blocks are independent: the results are identical)
static int32_t encode_slice(kz_ctx* ctx, const EncodePlan& p, int b0, int cnt, const HostPre* pre) {
  return kz_encode_blocks_pre(ctx, p.transformType, p.entropyType, p.blockSize, p.in + (int64_t)b0 * p.inStride, p.inStride, p.lengths + b0, cnt,
                              p.out + (int64_t)b0 * p.outStride, p.outStride, p.results + b0, p.memKind, pre);
}
// bound the scratch arena: the suffix sort needs ~43 B per input byte, so very large batches are processed as consecutive sub-batches
static int encode_max_batch(const EncodePlan& p) {
  bool hasBwt = false;
  ChainSpec noBwt = p.C.spec;
  for (int i = 0; i < noBwt.nb; i++) if (noBwt.types[i] == KZ_T_BWT) { hasBwt = true; noBwt.types[i] = KZ_T_NONE; }
  const size_t perBlock = pipeline_scratch(1, p.maxLen, false, noBwt) + (size_t)p.maxLen * 2 + 8192 + (size_t)(p.host ? p.outStride : 0) + (1 << 16);
  const size_t avail = hasBwt ? kz_arena_budget() / 2 : kz_arena_budget();      // the other half: suffix-sort groups
  return (int)std::min<size_t>(KZ_MAX_BATCH, std::max<size_t>(1, avail / perBlock));   // grid.y carries the block index
}
static int encode_split(kz_ctx* ctx, const EncodePlan& p, int maxB) {
  for (int b0 = 0; b0 < p.B; b0 += maxB) {
    const int cnt = std::min(maxB, p.B - b0);
    HostPre view;                                                   // a pre-staged batch is split like any other: every sub-batch sees its
    if (p.pre) view = p.pre->view(b0, cnt);                         // share of the host stages' results
    const int rc = encode_slice(ctx, p, b0, cnt, p.pre ? &view : nullptr);
    if (rc) return rc;
  }
  return 0;
}
// blocks per step of the encoder's host-stage pipeline: 256 for bulk batches; batches of a few dozen blocks (the silesia shape: 51)
// take thirds, so that the TEXT / UTF stages of all but the first third run under the GPU work of the third before
static int host_chunk_blocks(const kz_ctx* ctx, int B) {
  if (ctx->sw.hostChunk > 0) return ctx->sw.hostChunk < 8 ? 8 : ctx->sw.hostChunk;
  if (B >= 512) return 256;
  return std::max(12, (B + 2) / 3);
}
// Chains led by TEXT / UTF on large batches: the host stages of chunk k+1 run on a helper thread (and the host pool) while the GPU
// codes chunk k.  Blocks are independent, so chunking changes nothing in the output.
static int encode_host_chunk_pipeline(kz_ctx* ctx, const EncodePlan& p) {
  const int B = p.B, CH = host_chunk_blocks(ctx, B), nch = (B + CH - 1) / CH;
  struct Chunk { HostPre P; int rc = 0; };
  std::vector<Chunk> ck(nch);
  const int dev = ctx->device;
  for (int q = 0; q < 2; q++) {                                     // pinned, kept by the context: no fresh pages per chunk, DMA both ways
    int rc = kz_stage_reserve(ctx, ctx->hsOut[q], (size_t)host_pre_slot(p.maxLen) * (size_t)CH + 64, true);
    if (!rc && !p.host) rc = kz_stage_reserve(ctx, ctx->hsIn[q], (size_t)CH * (size_t)p.maxN + 64, true);
    if (rc) return rc;
  }
  const bool trace = ctx->sw.tracePipe != 0;
  const auto tStart = std::chrono::steady_clock::now();
  auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tStart).count(); };
  auto stage = [&](int k) {
    const double t0 = ms();
    const int b0 = k * CH, cnt = std::min(CH, B - b0);
    const uint8_t* hsrc = p.in + (int64_t)b0 * p.inStride;
    int64_t hstride = p.inStride;
    if (!p.host) {                                                  // device input: one copy back for the host stages (legacy stream:
      uint8_t* back = ctx->hsIn[k & 1].p;                           // it does not wait for the context's non-blocking stream)
      if (hipSetDevice(dev) != hipSuccess) { ck[k].rc = -KZ_ERR_DEVICE; return; }
      if (p.inStride == (int64_t)p.maxN) {
        if (hipMemcpy(back, hsrc, (size_t)cnt * (size_t)p.maxN, hipMemcpyDeviceToHost) != hipSuccess) { ck[k].rc = -KZ_ERR_DEVICE; return; }
      } else if (hipMemcpy2D(back, (size_t)p.maxN, hsrc, (size_t)p.inStride, (size_t)p.maxN, (size_t)cnt, hipMemcpyDeviceToHost) != hipSuccess) { ck[k].rc = -KZ_ERR_DEVICE; return; }
      hsrc = back; hstride = p.maxN;
    }
    const double t1 = ms();
    host_prestage(p.C, p.blockSize, p.maxLen, hsrc, hstride, p.lengths + b0, nullptr, cnt, ck[k].P, ctx->hsOut[k & 1].p);
    if (trace) fprintf(stderr, "[pipe] stage %d: copy back %.0f ms, host stages %.0f ms (at %.0f)\n", k, t1 - t0, ms() - t1, ms());
  };
  stage(0);
  for (int k = 0; k < nch; k++) {
    std::thread ahead;
    if (k + 1 < nch) ahead = std::thread(stage, k + 1);
    const int b0 = k * CH, cnt = std::min(CH, B - b0);
    int rc = ck[k].rc;
    const double tg = ms();
    if (!rc) rc = encode_slice(ctx, p, b0, cnt, &ck[k].P);
    ck[k].P = HostPre();
    const double tj = ms();
    if (ahead.joinable()) ahead.join();
    if (trace) fprintf(stderr, "[pipe] chunk %d: gpu %.0f ms, waited %.0f ms for the next stage (at %.0f)\n", k, tj - tg, ms() - tj, ms());
    if (rc) { if (rc == -KZ_ERR_DEVICE && !ctx->err[0]) snprintf(ctx->err, sizeof(ctx->err), "host stage: copy from the device failed"); return rc; }
  }
  return 0;
}

// ---- the one-pass path: named steps over one state ----
// where a block's bytes, skip bits and "dataType" entry come from once the host stages are through
struct BlockSrc {
  // Untouched: the caller's bytes, no stage looked at them.  Copy: a copy block (<= 15 bytes, or "skipBlocks" says so).  DeviceText: TEXT
  // applied on the device (length set there: TextCodec.java:667); UTF declines a block tagged TEXT (UTFCodec.java:93-101).  DeviceUtf: UTF
  // applied on the device (length set there), TEXT declined it.  Declined: every host stage declined it on the device, `dtype` is the entry
  // TEXT left.  HostPass: result `idx` of host pass `pass` beside / behind the device TEXT forward.  Pre: result `idx` of the host stages
  // run ahead (by the caller, or by this call).
  enum From { Untouched, Copy, DeviceText, DeviceUtf, Declined, HostPass, Pre } from = Untouched;
  int pass = -1, idx = -1;
  int dtype = KZ_DT_UNDEFINED;
};
struct EncodeState {
  const EncodePlan& p;
  Pipe P; FrameEnc F;
  u8* d_out = nullptr; kz_block_result* d_res = nullptr;
  std::vector<int32_t> h_copy, h_mask, h_applied, h_skip, h_threw;
  std::vector<BlockSrc> src;
  explicit EncodeState(const EncodePlan& p_) : p(p_), h_copy(p_.B), h_mask(p_.B), h_skip(p_.B, 0xFF), h_threw(p_.B, 0), src(p_.B) {}
};
// load blocks into HBM (device input: one strided copy kernel instead of one memcpy per block)
static int enc_load_blocks(kz_ctx* ctx, EncodeState& S) {
  const EncodePlan& p = S.p;
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  const int B = p.B;
  for (int b = 0; b < B; b++) bt.h_len[b] = p.lengths[b];
  KZ_HIP(hipMemcpyAsync(bt.d_len, p.lengths, (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (p.host) {
    for (int b = 0; b < B; b++) {
      if (p.lengths[b] == 0) continue;
      KZ_HIP(hipMemcpyAsync(bt.buf[0] + (int64_t)b * bt.stride, p.in + (int64_t)b * p.inStride, (size_t)p.lengths[b], hipMemcpyHostToDevice, st));
    }
  } else {
    pipe_copy_bytes(ctx, B, p.in, p.inStride, bt.buf[0], bt.stride, bt.d_len, nullptr, nullptr);
  }
  KZ_HIP(hipMemsetAsync(S.d_out, 0, (size_t)p.outStride * B, st));     // bit-concat ORs into zeroed words
  // the writer's per-block "dataType" tag from the first four bytes (CompressedOutputStream.java:795-804); the stages
  // that care (MM, LZ/LZX) read and update it on the device
  int rc = kz_block_data_types(ctx, bt, KZ_DT_UNDEFINED, true);
  if (rc) return rc;
  if (S.F.chk) { rc = kz_block_hashes(ctx, bt.buf[0], bt.stride, bt.d_len, B, S.F.chk, S.F.hash); if (rc) return rc; }
  return 0;
}
// which blocks the chain does not apply to (Sequence.forward, K/transform/Sequence.java:56-127, starts behind this)
static int enc_copy_decisions(kz_ctx* ctx, EncodeState& S) {
  const int B = S.p.B;
  hipStream_t st = ctx->stream;
  for (int b = 0; b < B; b++) S.h_copy[b] = (S.p.lengths[b] <= 15) ? 1 : 0;      // CompressedOutputStream.java:764-767
  if (ctx->skipBlocks) {                                                         // :769-788
    const int rc = kz_skip_block_flags(ctx, S.P.bt, S.P.d_applied);
    if (rc) return rc;
    KZ_HIP(hipMemcpyAsync(ctx->hpin, S.P.d_applied, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    KZ_HIP(kz_stream_sync(ctx, st));
    for (int b = 0; b < B; b++) if (ctx->hpin[b]) S.h_copy[b] = 1;
  }
  for (int b = 0; b < B; b++) if (S.h_copy[b]) S.src[b].from = BlockSrc::Copy;
  return 0;
}
// the device TEXT / UTF forward of a batch: what its two host passes share
struct DeviceFwd { TextFwdJob* J; std::vector<int32_t> take, keeps, declined; HostPre* pass; };
// one host pass over `blocks`: beside the device's walk (overlap: the walk is launched here) or behind it
static int enc_host_pass(kz_ctx* ctx, EncodeState& S, DeviceFwd& D, int pass, const std::vector<int>& blocks, bool overlap) {
  const EncodePlan& p = S.p;
  hipStream_t st = ctx->stream;
  kz_ctx::Stage& stg = ctx->tfIn;                                                // pinned staging for device input (not hsIn: ADVICE r5)
  std::vector<const uint8_t*> ptrs(blocks.size());
  std::vector<int32_t> lens(blocks.size()), firstStage(blocks.size(), 0), dtIn(blocks.size(), KZ_DT_UNDEFINED);
  if (!p.host && !blocks.empty()) {
    int r2 = kz_stage_reserve(ctx, stg, (size_t)blocks.size() * (size_t)p.maxN + 64, true);
    if (r2) return r2;
  }
  // the copies of a pass that runs beside the walk go on their own stream (the caller's input is not this context's to order:
  // k_copy_bytes read it on the main stream without waiting either), the walk is queued on the main one meanwhile
  if (overlap && !p.host && !ctx->tfCopy) KZ_HIP(hipStreamCreateWithFlags(&ctx->tfCopy, hipStreamNonBlocking));
  hipStream_t cs = (overlap && !p.host) ? ctx->tfCopy : st;
  for (size_t k = 0; k < blocks.size(); k++) {
    const int b = blocks[k];
    lens[k] = p.lengths[b];
    S.src[b].from = BlockSrc::HostPass; S.src[b].pass = pass; S.src[b].idx = (int)k;
    if (D.declined[b] >= 0) { firstStage[k] = 1; dtIn[k] = D.declined[b]; }      // TEXT is done with it
    if (p.host) ptrs[k] = p.in + (int64_t)b * p.inStride;
    else {
      ptrs[k] = stg.p + k * (size_t)p.maxN;
      KZ_HIP(hipMemcpyAsync(stg.p + k * (size_t)p.maxN, p.in + (int64_t)b * p.inStride, (size_t)p.lengths[b], hipMemcpyDeviceToHost, cs));
    }
  }
  if (overlap) {
    int r2 = kz_text_fwd_gpu_launch(ctx, S.P.bt, *D.J);
    if (r2) return r2;
    if (!p.host) KZ_HIP(hipStreamSynchronize(cs));
  } else KZ_HIP(kz_stream_sync(ctx, st));
  uint8_t* store = nullptr;                                                      // pinned slots for the stages' outputs, when there is room for them
  if (!blocks.empty() && kz_stage_reserve(ctx, ctx->tfOut[pass], (size_t)host_pre_slot(p.maxLen) * blocks.size() + 64, true) == 0) store = ctx->tfOut[pass].p;
  const auto t0 = std::chrono::steady_clock::now();
  host_prestage_list(p.C, p.blockSize, p.maxLen, ptrs, lens, D.pass[pass], store, &firstStage, &dtIn);
  if (ctx->sw.textGpuTrace)
    fprintf(stderr, "[textfwd%s] host pass %d: %d blocks, %.0f ms\n", kz_fast_coder((int)p.entropyType) ? "" : "1", pass, (int)blocks.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}
// TEXT forward on the device (kz_text_fwd_gpu.hip) for the blocks it keeps after its statistics and finishes: they are rewritten
// in their slots (hashes and Magic tags were taken from the original bytes, on the same stream).  The host stages run on
// the blocks it does not keep WHILE its walk runs, then on the few it kept and could not finish.
static int enc_device_forward(kz_ctx* ctx, EncodeState& S, HostPre* passP) {
  const EncodePlan& p = S.p;
  kz_batch& bt = S.P.bt;
  const int B = p.B, hp = p.C.hp;
  std::unique_ptr<TextFwdJob, void (*)(TextFwdJob*)> J(kz_text_fwd_gpu_new(), kz_text_fwd_gpu_free);
  DeviceFwd D{J.get(), std::vector<int32_t>(B), {}, std::vector<int32_t>(B, -1), passP};
  std::vector<int32_t> gpuDone(B, 0);
  for (int b = 0; b < B; b++) D.take[b] = (!S.h_copy[b] && p.lengths[b] > 0) ? 1 : 0;
  int rc = kz_text_fwd_gpu_classify(ctx, bt, p.blockSize, D.take, D.keeps, D.declined, *J, !kz_fast_coder((int)p.entropyType));
  if (rc) return rc;
  // a block that is not text: TEXT declined it on the device and left its "dataType"; UTF (if the chain has it) looks at UNDEFINED
  // and UTF8 blocks only (UTFCodec.java:93-101), on the host, from that entry on; every other block is done with the host stages
  for (int b = 0; b < B; b++)
    if (D.declined[b] >= 0 && (hp == 1 || (D.declined[b] != KZ_DT_UNDEFINED && D.declined[b] != KZ_DT_UTF8))) { S.src[b].from = BlockSrc::Declined; S.src[b].dtype = D.declined[b]; }
  // UTF forward on the device for the blocks TEXT declined as UTF-8 (kz_utf_fwd_gpu.hip; KZ_UTF_FWD_GPU=0: host stage): what it
  // finishes or declines by the reference's rules needs no host stage
  if (hp == 2 && ctx->sw.utfFwdGpu != 0) {
    std::vector<int32_t> takeU(B, 0), utfDone(B, 0);
    int nU = 0;
    for (int b = 0; b < B; b++) if (D.take[b] && D.declined[b] == KZ_DT_UTF8) { takeU[b] = 1; nU++; }
    if (nU) { rc = kz_utf_fwd_gpu(ctx, bt, takeU, utfDone); if (rc) return rc; }
    for (int b = 0; b < B; b++) if (utfDone[b]) { S.src[b].from = utfDone[b] == 1 ? BlockSrc::DeviceUtf : BlockSrc::Declined; S.src[b].dtype = D.declined[b]; }
  }
  std::vector<int> first, second;
  for (int b = 0; b < B; b++) if (D.take[b] && !D.keeps[b] && S.src[b].from != BlockSrc::Declined && S.src[b].from != BlockSrc::DeviceUtf) first.push_back(b);
  rc = enc_host_pass(ctx, S, D, 0, first, true);
  if (rc) return rc;
  rc = kz_text_fwd_gpu_finish(ctx, bt, *J, gpuDone);
  if (rc) return rc;
  for (int b = 0; b < B; b++) {
    if (gpuDone[b]) S.src[b].from = BlockSrc::DeviceText;
    else if (D.take[b] && D.keeps[b]) second.push_back(b);
  }
  if (!second.empty()) { rc = enc_host_pass(ctx, S, D, 1, second, false); if (rc) return rc; }
  return 0;
}
// the host stages of the whole batch in this call, from the caller's memory or a copy of it
static int enc_host_forward(kz_ctx* ctx, EncodeState& S, HostPre& mine) {
  const EncodePlan& p = S.p;
  const int B = p.B;
  std::unique_ptr<uint8_t[]> hostCopy;
  const uint8_t* hsrc = p.in;
  int64_t hstride = p.inStride;
  if (!p.host) {
    hostCopy.reset(new uint8_t[(size_t)B * (size_t)p.maxN + 64]);
    for (int b = 0; b < B; b++)
      if (p.lengths[b]) KZ_HIP(hipMemcpyAsync(hostCopy.get() + (size_t)b * p.maxN, p.in + (int64_t)b * p.inStride, (size_t)p.lengths[b], hipMemcpyDeviceToHost, ctx->stream));
    hsrc = hostCopy.get(); hstride = p.maxN;
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  }
  host_prestage(p.C, p.blockSize, p.maxLen, hsrc, hstride, p.lengths, S.h_copy.data(), B, mine);
  return 0;
}
// Host stages (TEXT, UTF): per block on host threads (ahead of this call when `pre` is given) or on the device; a block a stage
// applied to is replaced in HBM, its skip flag bits and its "dataType" entry (the writer's Magic tag, then whatever TEXT / UTF leave
// there) go on to the GPU stages
static int enc_host_stages(kz_ctx* ctx, EncodeState& S) {
  const EncodePlan& p = S.p;
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  const int B = p.B;
  hipEvent_t e0; kz_stage_begin(ctx, &e0);
  HostPre mine, passP[2];
  const HostPre* pre = p.pre;
  if (p.textFwdGpu) { const int rc = enc_device_forward(ctx, S, passP); if (rc) return rc; }
  else {
    if (!pre) { const int rc = enc_host_forward(ctx, S, mine); if (rc) return rc; pre = &mine; }
    for (int b = 0; b < B; b++) if (!S.h_copy[b]) { S.src[b].from = BlockSrc::Pre; S.src[b].idx = b; }   // (a pre-staged block of <= 15 bytes was left alone as well)
  }
  KZ_HIP(kz_stream_sync(ctx, st));                                              // the blocks are in HBM, hashed and tagged: slots may be rewritten
  std::vector<int32_t> dts(B, KZ_DT_UNDEFINED);
  for (int b = 0; b < B; b++) {
    const BlockSrc& s = S.src[b];
    const HostPre* q = nullptr;
    S.h_mask[b] = 0;
    switch (s.from) {
      case BlockSrc::Untouched: case BlockSrc::Copy: bt.h_len[b] = p.lengths[b]; continue;
      case BlockSrc::Declined: bt.h_len[b] = p.lengths[b]; dts[b] = s.dtype; continue;
      case BlockSrc::DeviceUtf: S.h_skip[b] = 0xFF & ~(1 << 6); dts[b] = KZ_DT_UTF8; continue;
      case BlockSrc::DeviceText: S.h_skip[b] = 0xFF & ~(1 << 7); dts[b] = KZ_DT_TEXT; continue;
      case BlockSrc::HostPass: q = &passP[s.pass]; break;
      case BlockSrc::Pre: q = pre; break;
    }
    const int k = s.idx;
    S.h_skip[b] = q->skip[k];
    dts[b] = q->dtype[k];
    bt.h_len[b] = q->outLen[k];
    if (q->changed[k] && q->outLen[k] > 0) {
      if (q->pinned) S.h_mask[b] = 1;
      else KZ_HIP(hipMemcpyAsync(bt.buf[0] + (int64_t)b * bt.stride, q->data(k), (size_t)q->outLen[k], hipMemcpyHostToDevice, st));
    }
  }
  KZ_HIP(hipMemcpyAsync(bt.d_len, bt.h_len.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (pre && pre->pinned) {                                                     // the stages' outputs sit in pinned slots: one gather kernel reads them in place
    const int rc = upload_mask(ctx, S.P, S.h_mask);
    if (rc) return rc;
    pipe_copy_bytes(ctx, B, pre->store, pre->slot, bt.buf[0], bt.stride, bt.d_len, nullptr, S.P.d_mask);
  }
  KZ_HIP(hipMemcpyAsync(bt.d_dtype, dts.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  KZ_HIP(kz_stream_sync(ctx, st));                                              // pageable sources; `mine` and `dts` are locals
  kz_stage_end(ctx, e0, KZ_STAGE_HOST_FWD, 0);
  return 0;
}
// RLT bounds its output by the length of the ARRAY it writes into (RLT.java:115).  In the reference's writer (one job, equal
// block sizes) Sequence.forward swaps its two buffers after every stage that was applied (Sequence.java:107-114): after an even
// number of applied stages RLT writes into the task's `buffer`, grown to Sequence.getMaxEncodedLength(blockSize)
// (CompressedOutputStream.java:793,806-811), after an odd number into `data`, max(blockSize + blockSize / 8, 256 KiB) bytes
// (:215-216) unless the stage needs more (Sequence.java:82-87).  blockSize: the context's when set, else the longest block.
static int rlt_dst_lengths(kz_ctx* ctx, EncodeState& S, int i) {
  const int B = S.p.B, bs = ctx->rltBlockSize;
  const int evenLen = seq_max_len(S.p.C.types, S.p.C.nb, bs);
  const int oddLen = std::max(std::max(bs + (bs >> 3), 256 * 1024), evenLen);
  std::vector<int32_t> h_end(B);
  for (int b = 0; b < B; b++) h_end[b] = (__builtin_popcount(~S.h_skip[b] & 0xFF & ~((1 << (8 - i)) - 1)) & 1) ? oddLen : evenLen;
  int32_t* d_end = kz_arena_array<int32_t>(ctx, B);
  if (!d_end) { snprintf(ctx->err, sizeof(ctx->err), "encode: arena overflow"); return -KZ_ERR_DEVICE; }
  KZ_HIP(hipMemcpyAsync(d_end, h_end.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));                            // h_end is a local
  S.P.bt.d_rltEnd = d_end;
  return 0;
}
// the GPU stages of the chain, one after the other over the blocks they apply to
static int enc_gpu_chain(kz_ctx* ctx, EncodeState& S) {
  const Chain& C = S.p.C;
  kz_batch& bt = S.P.bt;
  const int B = S.p.B, entropy = (int)S.p.entropyType;
  for (int i = C.hp; i < C.nb; i++) {
    for (int b = 0; b < B; b++) S.h_mask[b] = (!S.h_copy[b] && bt.h_len[b] > 0) ? 1 : 0;
    if (C.types[i] == KZ_T_NONE) { for (int b = 0; b < B; b++) if (S.h_mask[b]) S.h_skip[b] &= ~(1 << (7 - i)); continue; }
    hipEvent_t e0; kz_stage_begin(ctx, &e0);
    int64_t inBytes = 0; for (int b = 0; b < B; b++) if (S.h_mask[b]) inBytes += bt.h_len[b];
    const int type = C.types[i];
    if (type == KZ_T_RLT) { const int rc = rlt_dst_lengths(ctx, S, i); if (rc) return rc; }
    const int rc = run_stage(ctx, S.P, S.h_mask, S.h_applied, [&](kz_batch& x) { return run_transform_stage(ctx, x, type, true, 0, entropy); });
    if (rc) return rc;
    kz_stage_end(ctx, e0, stage_id(type, true), inBytes);
    for (int b = 0; b < B; b++) {
      if (S.h_applied[b] > 0) S.h_skip[b] &= ~(1 << (7 - i));
      else if (S.h_applied[b] < 0) S.h_threw[b] = 1;                // an exception in the reference: ERR_PROCESS_BLOCK for the block
    }
  }
  return 0;
}
// header sizes, then the entropy stage (EntropyEncoder.encode + dispose); copy blocks and NONE entropy: raw bytes (NullEntropyEncoder.java:66-81)
static int enc_entropy(kz_ctx* ctx, EncodeState& S) {
  const EncodePlan& p = S.p;
  const EntropyRow* E = p.C.E;
  Pipe& P = S.P; FrameEnc& F = S.F;
  kz_batch& bt = P.bt;
  hipStream_t st = ctx->stream;
  const int B = p.B;
  int rc;
  for (int b = 0; b < B; b++) if (S.h_copy[b]) S.h_skip[b] = 0x7F;               // NullTransform applies (NONE_TYPE chain)
  KZ_HIP(hipMemcpyAsync(F.skipFlags, S.h_skip.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  KZ_HIP(hipMemcpyAsync(F.isCopy, S.h_copy.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  F.postLen = bt.d_len;
  KZ_LAUNCH(ctx, KID_FRAME_PREPARE, k_frame_prepare, dim3((B + 255) / 256), dim3(256), F, B);
  hipEvent_t e0; kz_stage_begin(ctx, &e0);
  int64_t inBytes = 0; for (int b = 0; b < B; b++) inBytes += bt.h_len[b];
  if (E->encode) {
    // small copy blocks use NONE: mask them out of the ANS stage by zero length, then copy raw
    for (int b = 0; b < B; b++) S.h_mask[b] = S.h_copy[b] ? 0 : 1;
    rc = mask_lengths(ctx, P, S.h_mask);
    if (rc) return rc;
    std::vector<int32_t> saved = bt.h_len;
    for (int b = 0; b < B; b++) if (S.h_copy[b]) bt.h_len[b] = 0;
    rc = E->encode(ctx, bt, S.d_out, p.outStride, F.hdrBytes, F.bits);
    if (rc) return rc;
    if (E->overflow) {                                              // a block that outgrew its buffer fails
      std::vector<int32_t> ok(B);
      KZ_HIP(hipMemcpyAsync(ok.data(), bt.d_flag, (size_t)B * 4, hipMemcpyDeviceToHost, st));
      KZ_HIP(kz_stream_sync(ctx, st));
      for (int b = 0; b < B; b++) if (!S.h_copy[b] && !ok[b]) S.h_threw[b] = 1;
    }
    bt.h_len = saved;
    KZ_HIP(hipMemcpyAsync(bt.d_len, P.d_lenSave, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  }
  // raw payload for copy blocks (and all blocks when entropy is NONE)
  for (int b = 0; b < B; b++) S.h_mask[b] = (p.entropyType == KZ_E_NONE || S.h_copy[b]) ? 1 : 0;
  rc = upload_mask(ctx, P, S.h_mask);
  if (rc) return rc;
  pipe_copy_bytes(ctx, B, bt.buf[bt.cur], bt.stride, S.d_out, p.outStride, bt.d_len, F.hdrBytes, P.d_mask);
  // bits = 8*len for those blocks
  std::vector<int64_t> hb(B);
  if (p.entropyType == KZ_E_NONE) {
    for (int b = 0; b < B; b++) hb[b] = 8LL * bt.h_len[b];
    KZ_HIP(hipMemcpyAsync(F.bits, hb.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
  } else {
    for (int b = 0; b < B; b++) if (S.h_copy[b]) { hb[b] = 8LL * bt.h_len[b]; KZ_HIP(hipMemcpyAsync(F.bits + b, &hb[b], 8, hipMemcpyHostToDevice, st)); }
  }
  KZ_HIP(kz_stream_sync(ctx, st));                                              // hb is a local
  kz_stage_end(ctx, e0, KZ_STAGE_ENTROPY_ENC, inBytes);
  return 0;
}
// block header, raw fallback (CompressedOutputStream.java:861-985), and the results back to the caller
static int enc_frame_and_results(kz_ctx* ctx, EncodeState& S) {
  const EncodePlan& p = S.p;
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  const int B = p.B;
  hipEvent_t e0; kz_stage_begin(ctx, &e0);
  KZ_LAUNCH(ctx, KID_FRAME_DECIDE, k_frame_decide, dim3((B + 255) / 256), dim3(256), S.F, B);
  pipe_copy_bytes(ctx, B, bt.buf[bt.cur], bt.stride, S.d_out, p.outStride, bt.d_len, S.F.hdrBytes, S.F.fallback);
  KZ_LAUNCH(ctx, KID_FRAME_HEADER, k_frame_header, dim3((B + 255) / 256), dim3(256), S.F, S.d_out, p.outStride, S.d_res, B);
  kz_stage_end(ctx, e0, KZ_STAGE_FRAME_ENC, 0);
  KZ_HIP(hipMemcpyAsync(p.results, S.d_res, (size_t)B * sizeof(kz_block_result), hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  for (int b = 0; b < B; b++) if (S.h_threw[b]) { p.results[b].status = -KZ_ERR_PROCESS_BLOCK; p.results[b].bits = 0; p.results[b].length = 0; }
  if (p.host) {
    for (int b = 0; b < B; b++) {
      const size_t nbytes = (size_t)((p.results[b].bits + 7) >> 3);
      if (nbytes) KZ_HIP(hipMemcpyAsync(p.out + (int64_t)b * p.outStride, S.d_out + (int64_t)b * p.outStride, nbytes, hipMemcpyDeviceToHost, st));
    }
    KZ_HIP(kz_stream_sync(ctx, st));
  }
  KZ_HIP(hipGetLastError());
  kz_ktimer_flush(ctx);
  return 0;
}
static int encode_one_pass(kz_ctx* ctx, const EncodePlan& p) {
  EncodeState S(p);
  const int B = p.B;
  int64_t extra = (p.host ? (int64_t)p.outStride * B : 0) + (int64_t)B * (sizeof(kz_block_result) + 64) + (int64_t)B * 32 + 8192;
  if (p.textFwdGpu) {                   // the device TEXT forward runs first and gives its scratch back: it needs the larger of the two, not the sum
    const int64_t tf = (int64_t)kz_text_fwd_gpu_scratch(B, p.blockSize, p.maxLen, !kz_fast_coder((int)p.entropyType)), rest = (int64_t)pipeline_scratch(B, p.maxLen, false, p.C.spec);
    if (tf > rest) extra += tf - rest;
  }
  int rc = pipe_setup(ctx, S.P, B, p.maxLen, extra, false, p.C.spec);
  if (rc) return rc;
  S.d_out = p.host ? kz_arena_array<u8>(ctx, (size_t)p.outStride * B) : p.out;
  S.d_res = kz_arena_array<kz_block_result>(ctx, B);
  if (!frame_enc_alloc(ctx, B, p.C.nb, S.F) || !S.d_res || !S.d_out) { snprintf(ctx->err, sizeof(ctx->err), "encode: arena overflow"); return -KZ_ERR_DEVICE; }
  rc = enc_load_blocks(ctx, S);
  if (!rc) rc = enc_copy_decisions(ctx, S);
  if (!rc && p.C.hp > 0) rc = enc_host_stages(ctx, S);
  if (!rc) rc = enc_gpu_chain(ctx, S);
  if (!rc) rc = enc_entropy(ctx, S);
  if (!rc) rc = enc_frame_and_results(ctx, S);
  return rc;
}
int32_t kz_encode_blocks_pre(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                             const uint8_t* in, int64_t inStride, const int32_t* lengths, int32_t nBlocks,
                             uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind, const HostPre* pre) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  if (nBlocks <= 0) return 0;
  KZ_HIP(hipSetDevice(ctx->device));
  EncodePlan p{transformType, entropyType, blockSize, in, inStride, lengths, nBlocks, out, outStride, results, memKind, pre};
  const int rc = encode_plan(ctx, p);
  if (rc) return rc;
  // RLT's dst.length rule (rlt_dst_lengths) goes by the block size of the WHOLE call, also where the batch is split into sub-batches or chunks
  struct RltBsScope { kz_ctx* c; bool own; RltBsScope(kz_ctx* c_, int v) : c(c_), own(c_->rltBlockSize == 0) { if (own) c->rltBlockSize = v; }
                      ~RltBsScope() { if (own) c->rltBlockSize = 0; } } rltScope(ctx, std::max(1, ctx->blockSizeSet ? std::max(blockSize, p.maxN) : p.maxN));
  const int maxB = encode_max_batch(p);
  if (p.B > maxB) return encode_split(ctx, p, maxB);
  // (with "skipBlocks" the copy decision comes from the device and precedes the host stages: that case takes the one-pass path)
  if (p.C.hp > 0 && !pre && !ctx->skipBlocks && p.B >= 2 * host_chunk_blocks(ctx, p.B) && !p.textFwdGpu) return encode_host_chunk_pipeline(ctx, p);
  return encode_one_pass(ctx, p);
}

// TEXT sizes its hash map by the stream's block size and the decoder is told that size explicitly: an encoder that silently
// used the context's default would write blocks a decoder of another block size cannot read.  Chains with TEXT therefore need
// kz_ctx_set_block_size first (kz_compress and the Python / Java bindings do it).
int32_t encode_block_size(kz_ctx* ctx, uint64_t transformType) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  Chain C;
  chain_split(transformType, C);
  for (int i = 0; i < C.nb; i++)
    if (C.types[i] == KZ_T_TEXT && !ctx->blockSizeSet) {
      snprintf(ctx->err, sizeof(ctx->err), "chains with TEXT need the stream's block size: call kz_ctx_set_block_size first");
      return -KZ_ERR_MISSING_PARAM;
    }
  return ctx->blockSize;
}
extern "C" int32_t kz_encode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType,
                                    const uint8_t* in, int64_t inStride, const int32_t* lengths, int32_t nBlocks,
                                    uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind) {
  const int32_t bsz = encode_block_size(ctx, transformType);
  if (bsz < 0) return bsz;
  return kz_encode_blocks_pre(ctx, transformType, entropyType, bsz, in, inStride, lengths, nBlocks, out, outStride, results, memKind, nullptr);
}
