// kz_decode.hip -- the batched decoder: the codec span of DecodingTask.decodeBlock in front of Sequence.inverse, and the block-header kernel
#include "kz_pipe.h"

// =================================================================================================
// decode
struct FrameDec {
  int32_t* preLen; int32_t* skipFlags; int32_t* hdrBytes; int32_t* raw; int32_t* tcopy; int32_t* status;
  int64_t* bitOff; int64_t* bitEnd;
  u64* hashRef;          // [B] checksum stored in the block header
  int chk;
};
// CompressedInputStream.java:1025-1095 readBlockHeader
__global__ void k_frame_parse(const u8* __restrict__ in, int64_t inStride, const int64_t* __restrict__ bitLen, FrameDec F,
                              int nbFunctions, int maxTransformLength, int entropyNone, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const u8* p = in + (int64_t)b * inStride;
  const int64_t W = bitLen[b];
  int status = 0, preLen = 0, hdrBytes = 0, raw = 0, tcopy = 0;
  u32 skipFlags = 0;
  if (W == 0) { status = 0; }
  else if (W < 8) status = -KZ_ERR_BLOCK_SIZE;
  else {
    const u32 mode = p[0];
    bool hasSkip = false;
    if (mode & 0x80) {
      if (mode & 0x10) { tcopy = 1; if (nbFunctions > 4) hasSkip = true; else skipFlags = ((mode << 4) | 0x0F) & 0xFF; }
      else raw = 1;
    } else if (mode & 0x10) hasSkip = true;
    else skipFlags = ((mode << 4) | 0x0F) & 0xFF;
    const int dataSize = 1 + ((mode >> 5) & 3);
    hdrBytes = 1 + (hasSkip ? 1 : 0) + dataSize + 1;
    if (W < (int64_t)hdrBytes * 8) status = -KZ_ERR_BLOCK_SIZE;
    else {
      int idx = 1;
      if (hasSkip) skipFlags = p[idx++];
      for (int i = 0; i < dataSize; i++) preLen = (preLen << 8) | p[idx++];
      const u8 ck = p[idx++];
      const int cbytes = (F.chk == 1) ? 4 : (F.chk == 2 ? 8 : 0);
      if (cbytes && W >= (int64_t)(hdrBytes + cbytes) * 8) { u64 hv = 0; for (int k = 0; k < cbytes; k++) hv = (hv << 8) | p[idx++]; F.hashRef[b] = hv; }
      hdrBytes += cbytes;
      if (ck != kz_block_cksum(mode, skipFlags, (u32)preLen, (u64)W)) status = -KZ_ERR_CRC_CHECK;
      else if (W < (int64_t)hdrBytes * 8) status = -KZ_ERR_BLOCK_SIZE;
      else if (preLen < 0 || preLen > maxTransformLength) status = -KZ_ERR_READ_FILE;
      else if (((W + 7) >> 3) > (int64_t)preLen + hdrBytes) status = -KZ_ERR_BLOCK_SIZE;     // :1158-1164
      // raw bytes (copy block, "transformed copy", NONE entropy) are read with NullEntropyDecoder: a stream shorter than
      // the stated length makes the bit stream throw -> ERR_PROCESS_BLOCK (CompressedInputStream.java:1305-1316,1366-1371)
      else if (preLen > 0 && (raw || tcopy || entropyNone) && W < 8LL * ((int64_t)hdrBytes + preLen)) status = -KZ_ERR_PROCESS_BLOCK;
    }
  }
  if (status) { preLen = 0; }
  F.preLen[b] = preLen; F.skipFlags[b] = (int32_t)(raw ? 0xFF : skipFlags); F.hdrBytes[b] = hdrBytes;
  F.raw[b] = raw; F.tcopy[b] = tcopy; F.status[b] = status;
  F.bitOff[b] = 8LL * hdrBytes; F.bitEnd[b] = W;
}
__global__ void k_copy_payload(const u8* __restrict__ in, int64_t inStride, u8* __restrict__ dst, int64_t stride,
                               const int32_t* __restrict__ len, const int32_t* __restrict__ hdrBytes, const int32_t* __restrict__ cond) {
  const int b = blockIdx.y;
  if (!cond[b]) return;
  const int n = len[b];
  const u8* s = in + (int64_t)b * inStride + hdrBytes[b];
  u8* d = dst + (int64_t)b * stride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) d[i] = s[i];
}

static bool frame_dec_alloc(kz_ctx* ctx, int B, FrameDec& F) {
  F.preLen = kz_arena_array<int32_t>(ctx, B); F.skipFlags = kz_arena_array<int32_t>(ctx, B); F.hdrBytes = kz_arena_array<int32_t>(ctx, B);
  F.raw = kz_arena_array<int32_t>(ctx, B); F.tcopy = kz_arena_array<int32_t>(ctx, B); F.status = kz_arena_array<int32_t>(ctx, B);
  F.bitOff = kz_arena_array<int64_t>(ctx, B); F.bitEnd = kz_arena_array<int64_t>(ctx, B); F.hashRef = kz_arena_array<u64>(ctx, B);
  F.chk = ctx->checksum;
  return F.preLen && F.skipFlags && F.hdrBytes && F.raw && F.tcopy && F.status && F.bitOff && F.bitEnd && F.hashRef;
}

// the caller's arguments
struct DecodeCall {
  uint32_t entropyType; int32_t blockSize;
  const uint8_t* in; int64_t inStride; const int64_t* bitLengths; int B;
  uint8_t* out; int64_t outStride; kz_block_result* results; int32_t memKind;
  DecodeCall slice(int b0, int cnt) const {         // blocks [b0, b0 + cnt) as a call of their own
    return DecodeCall{entropyType, blockSize, in + (int64_t)b0 * inStride, inStride, bitLengths + b0, cnt, out + (int64_t)b0 * outStride, outStride, results + b0, memKind};
  }
};
// sizes and device-stage choices of one batch.  deferHost: leave the host stages (TEXT / UTF inverse) to the caller: the blocks come
// out as the GPU chain left them, results[b] carry their skip flags and lengths (decode_host_chunk_pipeline runs those stages on a
// helper thread under the next chunk's GPU work).
struct DecodePlan {
  bool host, deferHost;
  int dataCap, maxTL, maxLen; int64_t maxInBytes;
  bool textGpu, utfGpu; int iu;                     // TEXT / UTF inverse on the device; iu: UTF as the host stage undone first (-1: none)
};
static DecodePlan decode_plan(const kz_ctx* ctx, const Chain& C, const DecodeCall& c, bool deferHost) {
  DecodePlan p;
  p.host = c.memKind == KZ_MEM_HOST; p.deferHost = deferHost;
  // decoder's working size: blockSize + max(512, blockSize/16) (CompressedInputStream.java:694-695)
  p.dataCap = c.blockSize + std::max(512, c.blockSize >> 4);
  p.maxTL = std::min(std::max(c.blockSize + c.blockSize / 2, 2048), 1 << 30);
  p.maxInBytes = 0;
  for (int b = 0; b < c.B; b++) p.maxInBytes = std::max(p.maxInBytes, (c.bitLengths[b] + 7) >> 3);
  // The reference accepts preTransformLength up to 1.5 x blockSize (CompressedInputStream.java:1139-1140);
  // no chain in scope expands a block by more than 1024 bytes, so buffers are sized dataCap+1024 and a
  // larger (corrupt) length is rejected with the same error code.
  p.maxLen = std::min(p.maxTL, p.dataCap + 1024);
  p.textGpu = C.hp > 0 && !deferHost && C.types[0] == KZ_T_TEXT && text_gpu_on(ctx, c.entropyType, c.B);
  p.iu = (C.hp > 0 && C.types[C.hp - 1] == KZ_T_UTF) ? C.hp - 1 : -1;
  p.utfGpu = p.iu >= 0 && !deferHost && utf_gpu_on(ctx);
  return p;
}
struct DecodeState {
  const Chain& C; const DecodeCall& c; const DecodePlan& p;
  Pipe P; FrameDec F;
  const u8* d_in = nullptr; int64_t inS = 0;
  u64* d_hashOut = nullptr; int64_t* d_bitLen = nullptr;
  std::vector<int32_t> h_skip, h_raw, h_tc, h_status, h_mask, h_applied;
};
// host streams: (bits + 7) / 8 bytes of each into a slot of the library's own
static int dec_stage_input(kz_ctx* ctx, DecodeState& S) {
  const DecodeCall& c = S.c;
  S.d_in = c.in;
  if (!S.p.host) return 0;
  u8* t = kz_arena_array<u8>(ctx, (size_t)S.inS * c.B);
  if (!t) { snprintf(ctx->err, sizeof(ctx->err), "decode: arena overflow"); return -KZ_ERR_DEVICE; }
  for (int b = 0; b < c.B; b++) {
    const size_t nbytes = (size_t)((c.bitLengths[b] + 7) >> 3);
    if (nbytes) KZ_HIP(hipMemcpyAsync(t + (int64_t)b * S.inS, c.in + (int64_t)b * c.inStride, nbytes, hipMemcpyHostToDevice, ctx->stream));
  }
  S.d_in = t;
  return 0;
}
// the block headers, parsed on the device and read back
static int dec_parse_frames(kz_ctx* ctx, DecodeState& S) {
  const int B = S.c.B;
  kz_batch& bt = S.P.bt;
  FrameDec& F = S.F;
  hipStream_t st = ctx->stream;
  S.d_hashOut = kz_arena_array<u64>(ctx, B);
  S.d_bitLen = kz_arena_array<int64_t>(ctx, B);
  if (!S.d_hashOut || !S.d_bitLen) { snprintf(ctx->err, sizeof(ctx->err), "decode: arena overflow"); return -KZ_ERR_DEVICE; }
  KZ_HIP(hipMemcpyAsync(S.d_bitLen, S.c.bitLengths, (size_t)B * 8, hipMemcpyHostToDevice, st));
  hipEvent_t e0; kz_stage_begin(ctx, &e0);
  KZ_LAUNCH(ctx, KID_FRAME_PARSE, k_frame_parse, dim3((B + 255) / 256), dim3(256), S.d_in, S.inS, S.d_bitLen, F, S.C.nb, S.p.maxLen, (S.c.entropyType == KZ_E_NONE) ? 1 : 0, B);
  // read back descriptors
  int32_t* hpb = ctx->hpin + 4 * B;
  const int32_t* const back[5] = {F.preLen, F.skipFlags, F.raw, F.tcopy, F.status};
  for (int k = 0; k < 5; k++) KZ_HIP(hipMemcpyAsync(hpb + k * B, back[k], (size_t)B * 4, hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  kz_stage_end(ctx, e0, KZ_STAGE_FRAME_DEC, 0);
  S.h_skip.assign(hpb + B, hpb + 2 * B); S.h_raw.assign(hpb + 2 * B, hpb + 3 * B); S.h_tc.assign(hpb + 3 * B, hpb + 4 * B); S.h_status.assign(hpb + 4 * B, hpb + 5 * B);
  for (int b = 0; b < B; b++) bt.h_len[b] = S.h_status[b] ? 0 : hpb[b];
  KZ_HIP(hipMemcpyAsync(bt.d_len, bt.h_len.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  S.h_mask.assign(B, 0);
  return 0;
}
// one pass of the entropy stage over the blocks of `part` (all blocks when null): entropy decode into buf
static int dec_entropy_pass(kz_ctx* ctx, DecodeState& S, const std::vector<int32_t>* part, const int32_t* d_part) {
  const int B = S.c.B;
  const EntropyRow* E = S.C.E;
  kz_batch& bt = S.P.bt;
  hipEvent_t e1; kz_stage_begin(ctx, &e1);
  int64_t outBytes = 0;
  std::vector<int32_t> h_rawp(B);
  for (int b = 0; b < B; b++) {
    const bool in = !part || (*part)[b];
    if (in) outBytes += bt.h_len[b];
    h_rawp[b] = (in && (S.c.entropyType == KZ_E_NONE || S.h_raw[b] || S.h_tc[b])) ? 1 : 0;
  }
  if (E->decode) {
    for (int b = 0; b < B; b++) S.h_mask[b] = ((!part || (*part)[b]) && !(S.h_raw[b] || S.h_tc[b])) ? 1 : 0;
    int r = run_stage(ctx, S.P, S.h_mask, S.h_applied, [&](kz_batch& x) { return E->decode(ctx, x, S.d_in, S.inS, S.F.bitOff, S.F.bitEnd); }, d_part);
    if (r) return r;
    for (int b = 0; b < B; b++) if (S.h_mask[b] && !S.h_applied[b] && !S.h_status[b]) S.h_status[b] = -KZ_ERR_PROCESS_BLOCK;
  } else {
    bt.cur ^= 1;    // raw path writes into the "next" buffer below
  }
  int r = upload_mask(ctx, S.P, h_rawp);
  if (r) return r;
  KZ_LAUNCH(ctx, KID_COPY_PAYLOAD, k_copy_payload, dim3(64, B), dim3(256), S.d_in, S.inS, bt.buf[bt.cur], bt.stride, bt.d_len, S.F.hdrBytes, S.P.d_mask);
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));                      // h_rawp is a local
  kz_stage_end(ctx, e1, KZ_STAGE_ENTROPY_DEC, outBytes);
  return 0;
}
// one inverse transform stage over the blocks of `part`
static int dec_transform_pass(kz_ctx* ctx, DecodeState& S, int i, const std::vector<int32_t>* part, const int32_t* d_part) {
  const int B = S.c.B, type = S.C.types[i];
  kz_batch& bt = S.P.bt;
  bool any = false;
  for (int b = 0; b < B; b++) {
    S.h_mask[b] = ((!part || (*part)[b]) && !S.h_status[b] && !(S.h_skip[b] & (1 << (7 - i))) && bt.h_len[b] > 0) ? 1 : 0;
    any |= S.h_mask[b] != 0;
  }
  if (!any && !part) return 0;
  hipEvent_t e1; kz_stage_begin(ctx, &e1);
  int r = run_stage(ctx, S.P, S.h_mask, S.h_applied, [&](kz_batch& x) { return run_transform_stage(ctx, x, type, false, S.p.dataCap, (int)S.c.entropyType); }, d_part);
  if (r) return r;
  int64_t outBytes = 0; for (int b = 0; b < B; b++) if (S.h_mask[b]) outBytes += bt.h_len[b];
  kz_stage_end(ctx, e1, stage_id(type, false), outBytes);
  for (int b = 0; b < B; b++) if (S.h_mask[b] && !S.h_applied[b]) { S.h_status[b] = -KZ_ERR_PROCESS_BLOCK; bt.h_len[b] = 0; }
  return 0;
}
// "Expensive blocks first" for BWT+RANK+ZRLT (or MTFT) chains on large batches: the RANK inverse of a block is serial and
// its cost (the ZRLT-coded length = the decoded length, known from the block header) differs by an order of magnitude
// between blocks.  The expensive blocks go through entropy decoding and ZRLT inverse FIRST and start their RANK inverse on
// the side stream; the others follow on the main stream underneath it (kz_overlap.hip).  Returns 1 when it ran the whole chain,
// 0 when the schedule does not apply, <0 on error.
static int dec_expensive_first(kz_ctx* ctx, DecodeState& S) {
  const Chain& C = S.C;
  const int B = S.c.B, hp = C.hp;
  kz_batch& bt = S.P.bt;
  if (!(C.nb - hp == 3 && C.types[hp] == KZ_T_BWT && (C.types[hp + 1] == KZ_T_RANK || C.types[hp + 1] == KZ_T_MTFT) && C.types[hp + 2] == KZ_T_ZRLT &&
        (S.c.entropyType == KZ_E_ANS0 || S.c.entropyType == KZ_E_HUFFMAN) && !ctx->sw.noSFirst)) return 0;
  bool all = true;
  const int need = (1 << (7 - hp)) | (1 << (7 - (hp + 1)));       // BWT and RANK applied to every block
  for (int b = 0; b < B && all; b++) all = !S.h_status[b] && bt.h_len[b] > 0 && !(S.h_skip[b] & need);   // (copy blocks carry all skip bits)
  Overlap O;
  std::vector<int32_t> ones(B, 1);
  if (ctx->sw.traceSched) {
    int nst = 0, ntc = 0, nz = 0, nsk = 0, nraw = 0;
    for (int b = 0; b < B; b++) { nst += S.h_status[b] != 0; ntc += S.h_tc[b] != 0; nz += bt.h_len[b] <= 0; nsk += (S.h_skip[b] & need) != 0; nraw += S.h_raw[b] != 0; }
    fprintf(stderr, "[sched] B=%d all=%d status=%d tcopy=%d empty=%d skipBwtRank=%d raw=%d\n", B, (int)all, nst, ntc, nz, nsk, nraw);
  }
  // cost of a block's RANK inverse: its COMPRESSED size.  The time per rank grows with the rank (positions shifted), and so
  // does the entropy coder's output; the ZRLT-coded length alone puts skewed and uniform data in one class (68 vs 134 ns / rank)
  std::vector<int32_t> cost(B);
  for (int b = 0; b < B; b++) cost[b] = (int32_t)std::min<int64_t>((S.c.bitLengths[b] + 7) >> 3, 0x7FFFFFFF);
  if (!all || !overlap_classify(ctx, B, ones, cost, O)) return 0;
  const int mode = C.types[hp + 1] == KZ_T_RANK ? 2 : 1;
  int rc = overlap_alloc(ctx, B, O);
  if (rc) return rc;
  bt.h_cost = cost;
  {
    std::vector<int32_t> rawp(B);
    for (int b = 0; b < B; b++) rawp[b] = (S.h_raw[b] || S.h_tc[b]) ? 1 : 0;
    overlap_plan(ctx, O, bt.h_len, rawp, S.c.blockSize, true);
  }
  for (size_t k = 0; k < O.launchOrder.size(); k++) {
    const int g = O.launchOrder[k];
    rc = dec_entropy_pass(ctx, S, &O.groups[g].in, O.groups[g].d_in);
    if (!rc) rc = dec_transform_pass(ctx, S, hp + 2, &O.groups[g].in, O.groups[g].d_in);
    if (!rc) rc = overlap_start_rank(ctx, bt, mode, O, g, (int)k);
    if (rc) return rc;
  }
  rc = overlap_finish(ctx, S.P, O, S.h_applied);
  if (rc) return rc;
  for (int b = 0; b < B; b++) if (!S.h_status[b] && !S.h_applied[b]) { S.h_status[b] = -KZ_ERR_PROCESS_BLOCK; bt.h_len[b] = 0; }
  return 1;
}
// the plain path: entropy decoding, then the inverse chain (Sequence.inverse, K/transform/Sequence.java:137-207)
static int dec_inverse_chain(kz_ctx* ctx, DecodeState& S) {
  const Chain& C = S.C;
  const int B = S.c.B, hp = C.hp;
  kz_batch& bt = S.P.bt;
  int rc = dec_entropy_pass(ctx, S, nullptr, nullptr);
  if (rc) return rc;
  // cost hint for the serial-per-block inverse stages: the length a block had at the input of the previous stage
  // (for RANK behind ZRLT that is the ZRLT-coded length ~ the number of non-zero ranks)
  std::vector<int32_t> prevIn(B);
  for (int b = 0; b < B; b++) prevIn[b] = (int32_t)std::min<int64_t>((S.c.bitLengths[b] + 7) >> 3, 0x7FFFFFFF);
  for (int i = C.nb - 1; i >= hp; i--) {
    if (C.types[i] == KZ_T_NONE) continue;
    bt.h_cost = prevIn;
    prevIn = bt.h_len;
    bool any = false;
    for (int b = 0; b < B; b++) { S.h_mask[b] = (!S.h_status[b] && !(S.h_skip[b] & (1 << (7 - i))) && bt.h_len[b] > 0) ? 1 : 0; any |= S.h_mask[b] != 0; }
    if (!any) continue;
    const int type = C.types[i];
    if ((type == KZ_T_RANK || type == KZ_T_MTFT) && i - 1 >= hp && C.types[i - 1] == KZ_T_BWT) {
      // RANK / MTFT inverse followed by the BWT inverse on the same blocks: overlapped schedule for large batches
      bool same = true;
      for (int b = 0; b < B && same; b++) same = ((S.h_skip[b] >> (7 - i)) & 1) == ((S.h_skip[b] >> (8 - i)) & 1);
      if (same) {
        const int fr = overlapped_rank_bwt_inverse(ctx, S.P, type == KZ_T_RANK ? 2 : 1, S.h_mask, bt.h_cost, S.h_applied);
        if (fr < 0) return fr;
        if (fr > 0) {
          for (int b = 0; b < B; b++) if (S.h_mask[b] && !S.h_applied[b]) { S.h_status[b] = -KZ_ERR_PROCESS_BLOCK; bt.h_len[b] = 0; }
          prevIn = bt.h_len;
          i--;                                                        // the BWT stage is done as well
          continue;
        }
      }
    }
    rc = dec_transform_pass(ctx, S, i, nullptr, nullptr);
    if (rc) return rc;
  }
  return 0;
}
// the inverses of UTF and TEXT on the device for the blocks that went through them; h_skipHost: the host stages' view (a stage
// counts as skipped for the blocks the device took)
static int dec_device_host_inverses(kz_ctx* ctx, DecodeState& S, std::vector<int32_t>& h_skipHost) {
  const int B = S.c.B, hp = S.C.hp, iu = S.p.iu;
  kz_batch& bt = S.P.bt;
  if (S.p.utfGpu) {
    // blocks that went through UTF (the host stage undone first): its inverse on the device
    std::vector<int32_t> take(B, 0), done;
    for (int b = 0; b < B; b++) take[b] = (!S.h_status[b] && bt.h_len[b] > 0 && !(S.h_skip[b] & (1 << (7 - iu)))) ? 1 : 0;
    hipEvent_t e0; kz_stage_begin(ctx, &e0);
    const int rc = kz_stage_utf_inverse_gpu(ctx, bt, S.p.dataCap, take, done);
    if (rc) return rc;
    kz_stage_end(ctx, e0, KZ_STAGE_HOST_INV, 0);
    for (int b = 0; b < B; b++) if (done[b]) h_skipHost[b] |= 1 << (7 - iu);
  }
  if (S.p.textGpu) {
    // blocks whose only host stage left is TEXT (every other host stage skipped for the block, or done above): its inverse on the device
    std::vector<int32_t> take(B, 0), done;
    for (int b = 0; b < B; b++) {
      bool t = !S.h_status[b] && bt.h_len[b] > 0 && !(S.h_skip[b] & 0x80);
      for (int i = 1; i < hp && t; i++) t = (h_skipHost[b] & (1 << (7 - i))) != 0;
      take[b] = t ? 1 : 0;
    }
    hipEvent_t e0; kz_stage_begin(ctx, &e0);
    const int rc = kz_stage_text_inverse_gpu(ctx, bt, S.c.blockSize, S.p.dataCap, !kz_fast_coder((int)S.c.entropyType), take, done, text_gpu_form(ctx, S.c.entropyType, B));
    if (rc) return rc;
    kz_stage_end(ctx, e0, KZ_STAGE_HOST_INV, 0);
    for (int b = 0; b < B; b++) if (done[b]) h_skipHost[b] |= 0x80;
  }
  return 0;
}
// host stages (UTF, TEXT inverse) behind the GPU stages: blocks that went through one come back to the host, are decoded
// on host threads and return to their slot
static int dec_host_inverses(kz_ctx* ctx, DecodeState& S, const std::vector<int32_t>& h_skipHost) {
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  hipEvent_t e1; kz_stage_begin(ctx, &e1);
  KZ_HIP(kz_stream_sync(ctx, st));
  HostInv H;
  host_inv_make(H, ctx, S.C, S.c.blockSize, S.p.dataCap, bt.buf[bt.cur], bt.stride, false, bt.h_len.data(), h_skipHost.data(), S.h_status.data());
  kz_parallel_for(S.c.B, KZ_HOST_STAGE_THREADS, host_inverse_block, &H);
  if (H.fail) { snprintf(ctx->err, sizeof(ctx->err), "host stage: copy from / to the device failed"); return -KZ_ERR_DEVICE; }
  KZ_HIP(hipMemcpyAsync(bt.d_len, bt.h_len.data(), (size_t)S.c.B * 4, hipMemcpyHostToDevice, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  kz_stage_end(ctx, e1, KZ_STAGE_HOST_INV, 0);
  return 0;
}
// checksum verification (CompressedInputStream.java:1349-1363)
static int dec_verify_checksums(kz_ctx* ctx, DecodeState& S) {
  const int B = S.c.B;
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  const int rc = kz_block_hashes(ctx, bt.buf[bt.cur], bt.stride, bt.d_len, B, S.F.chk, S.d_hashOut);
  if (rc) return rc;
  std::vector<u64> h1(B), h2(B);
  KZ_HIP(hipMemcpyAsync(h1.data(), S.F.hashRef, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  KZ_HIP(hipMemcpyAsync(h2.data(), S.d_hashOut, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  for (int b = 0; b < B; b++) if (!S.h_status[b] && bt.h_len[b] > 0 && h1[b] != h2[b]) S.h_status[b] = -KZ_ERR_CRC_CHECK;
  return 0;
}
static int dec_write_results(kz_ctx* ctx, DecodeState& S) {
  const DecodeCall& c = S.c;
  const int B = c.B;
  kz_batch& bt = S.P.bt;
  hipStream_t st = ctx->stream;
  for (int b = 0; b < B; b++) {
    if (!S.h_status[b] && (bt.h_len[b] > c.outStride || (!S.p.deferHost && bt.h_len[b] > c.blockSize))) S.h_status[b] = -KZ_ERR_PROCESS_BLOCK;
    c.results[b].bits = c.bitLengths[b]; c.results[b].length = S.h_status[b] ? 0 : bt.h_len[b]; c.results[b].status = S.h_status[b];
    c.results[b].skipFlags = (uint8_t)S.h_skip[b]; c.results[b].mode = 0;
    if (S.p.host && !S.h_status[b] && bt.h_len[b] > 0)
      KZ_HIP(hipMemcpyAsync(c.out + (int64_t)b * c.outStride, bt.buf[bt.cur] + (int64_t)b * bt.stride, (size_t)bt.h_len[b], hipMemcpyDeviceToHost, st));
  }
  if (!S.p.host) {                                               // device output: one strided copy kernel (failed blocks: length 0)
    for (int b = 0; b < B; b++) ctx->hpin[b] = S.h_status[b] ? 0 : bt.h_len[b];
    KZ_HIP(hipMemcpyAsync(bt.d_len, ctx->hpin, (size_t)B * 4, hipMemcpyHostToDevice, st));
    pipe_copy_bytes(ctx, B, bt.buf[bt.cur], bt.stride, c.out, c.outStride, bt.d_len, nullptr, nullptr);
  }
  KZ_HIP(kz_stream_sync(ctx, st));
  KZ_HIP(hipGetLastError());
  kz_ktimer_flush(ctx);
  return 0;
}
static int decode_one_pass(kz_ctx* ctx, const Chain& C, const DecodeCall& c, const DecodePlan& p) {
  DecodeState S{C, c, p};
  const int B = c.B;
  S.inS = p.host ? (int64_t)kz_align((size_t)p.maxInBytes + 64, 256) : c.inStride;
  // (the expensive-blocks-first schedule runs the entropy and ZRLT stages once per group: a second set of their small scratch)
  const int64_t extra = (p.host ? S.inS * B : 0) + (int64_t)B * (sizeof(kz_block_result) + 128) + (int64_t)B * 32 + 8192 +
                        (int64_t)kz_zrlt_scratch(B, p.maxLen) + (int64_t)B * ((int64_t)(p.maxLen / 16384 + 4) * 8 + 64) + 65536 + (int64_t)B * 64 +
                        (p.textGpu ? (int64_t)B * (int64_t)kz_text_gpu_scratch_per_block(c.blockSize) + (int64_t)B * 16 + (1 << 16) : 0) +
                        (p.utfGpu ? (int64_t)B * (int64_t)kz_utf_gpu_scratch_per_block(p.maxLen) + (int64_t)B * 16 + (1 << 16) : 0);
  int rc = pipe_setup(ctx, S.P, B, p.maxLen, extra, true, C.spec);
  if (!rc) rc = dec_stage_input(ctx, S);
  if (rc) return rc;
  if (!frame_dec_alloc(ctx, B, S.F)) { snprintf(ctx->err, sizeof(ctx->err), "decode: arena overflow"); return -KZ_ERR_DEVICE; }
  rc = dec_parse_frames(ctx, S);
  if (rc) return rc;
  rc = dec_expensive_first(ctx, S);
  if (rc < 0) return rc;
  if (rc == 0) { rc = dec_inverse_chain(ctx, S); if (rc) return rc; }
  std::vector<int32_t> h_skipHost(S.h_skip);
  rc = dec_device_host_inverses(ctx, S, h_skipHost);
  if (!rc && C.hp > 0 && !p.deferHost) rc = dec_host_inverses(ctx, S, h_skipHost);
  if (!rc && S.F.chk) rc = dec_verify_checksums(ctx, S);
  if (!rc) rc = dec_write_results(ctx, S);
  return rc;
}
static int32_t decode_blocks_impl(kz_ctx* ctx, const Chain& C, const DecodeCall& c, bool deferHost);
// bound the arena: very large batches are decoded as consecutive sub-batches.  Returns 0 when the batch fits (nothing done), 1 when it
// was decoded in parts, <0 on error.
static int decode_split(kz_ctx* ctx, const Chain& C, const DecodeCall& c, const DecodePlan& p) {
  const size_t perBlock = pipeline_scratch(1, p.maxLen, true, C.spec) + (size_t)p.maxLen * 2 + (size_t)(p.host ? p.maxInBytes : 0) + (1 << 16) +
                          (p.textGpu ? kz_text_gpu_scratch_per_block(c.blockSize) : 0) + (p.utfGpu ? kz_utf_gpu_scratch_per_block(p.maxLen) : 0);
  int maxB = (int)std::min<size_t>(KZ_MAX_BATCH, std::max<size_t>(1, kz_arena_budget() / perBlock));   // grid.y carries the block index
  // the serial-per-block inverse stages like whole multiples of 8 blocks per CU (one wave per block, two per SIMD)
  const int unit = 8 * (ctx->numCUs > 0 ? ctx->numCUs : 256);
  if (c.B > maxB && maxB > unit) maxB = (maxB / unit) * unit;       // only when the batch has to be split anyway
  if (c.B <= maxB) return 0;
  for (int b0 = 0; b0 < c.B; b0 += maxB) {
    const int rc = decode_blocks_impl(ctx, C, c.slice(b0, std::min(maxB, c.B - b0)), p.deferHost);
    if (rc) return rc;
  }
  return 1;
}
static int32_t decode_blocks_impl(kz_ctx* ctx, const Chain& C, const DecodeCall& c, bool deferHost) {
  const DecodePlan p = decode_plan(ctx, C, c, deferHost);
  const int split = decode_split(ctx, C, c, p);
  return split ? std::min(split, 0) : decode_one_pass(ctx, C, c, p);
}

static void decode_error_sync(kz_ctx* ctx) {
  // an error exit may leave kernels of the overlapped schedule running on the side streams: the next call reuses (or frees) the
  // arena they work in
  for (int i = 0; i < 5; i++) if (ctx->side[i]) hipStreamSynchronize(ctx->side[i]);
  hipStreamSynchronize(ctx->stream);
}
static int set_device(kz_ctx* ctx) { KZ_HIP(hipSetDevice(ctx->device)); return 0; }
// Chains led by TEXT / UTF on large batches: the host inverse stages of chunk k run on a helper thread (and the host pool)
// while the GPU decodes chunk k+1.
static int decode_host_chunk_pipeline(kz_ctx* ctx, const Chain& C, const DecodeCall& c, const DecodePlan& p) {
  const int CH = ctx->sw.hostChunkDec, B = c.B, nch = (B + CH - 1) / CH;
  std::vector<std::thread> finishers;
  std::vector<std::unique_ptr<HostInv>> jobs;
  std::vector<std::vector<int32_t>> lens(nch), skips(nch), stats(nch);
  int rc = 0;
  const bool trace = ctx->sw.tracePipe != 0;
  // KZ_HOST_INV_STAGED=1: the chunk's blocks go through pinned slots with one gather / scatter kernel per
  // sub-chunk instead of a copy pair per block.  Measured slower on the level-exact bench row (1 200 vs 1 066 ms per 2 048-block
  // decode), so it is opt-in.
  const bool staged = ctx->sw.hostInvStaged == 1 && !p.host;
  const int64_t pslot = (int64_t)kz_align((size_t)std::max<int64_t>(c.outStride, p.dataCap) + 64, 64);
  if (staged) {                                                     // everything that can fail, before the first chunk is in flight
    for (int q = 0; q < 2 && !rc; q++) {
      rc = kz_stage_reserve(ctx, ctx->hsIn[q], (size_t)pslot * (size_t)CH + 64, true);
      if (!rc) rc = kz_stage_reserve(ctx, ctx->hiAux[q], (size_t)CH * 16 + 64, false);
      if (!rc && !ctx->hiStream[q] && hipStreamCreateWithFlags(&ctx->hiStream[q], hipStreamNonBlocking) != hipSuccess) rc = -KZ_ERR_DEVICE;
    }
    if (rc) return rc;
  }
  const auto tz = std::chrono::steady_clock::now();
  auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tz).count(); };
  for (int k = 0; k < nch && !rc; k++) {
    const int b0 = k * CH, cnt = std::min(CH, B - b0);
    const double tg = ms();
    rc = decode_blocks_impl(ctx, C, c.slice(b0, cnt), true);
    if (trace) fprintf(stderr, "[pipe] decode chunk %d: gpu %.0f ms (at %.0f)\n", k, ms() - tg, ms());
    if (rc) break;
    lens[k].resize(cnt); skips[k].resize(cnt); stats[k].resize(cnt);
    for (int i = 0; i < cnt; i++) { lens[k][i] = c.results[b0 + i].length; skips[k][i] = c.results[b0 + i].skipFlags; stats[k][i] = c.results[b0 + i].status; }
    jobs.emplace_back(new HostInv());
    HostInv* H = jobs.back().get();
    host_inv_make(*H, ctx, C, c.blockSize, p.dataCap, c.out + (int64_t)b0 * c.outStride, c.outStride, p.host, lens[k].data(), skips[k].data(), stats[k].data());
    if (staged) {                                                   // ring of two pinned slot sets: chunk k - 2 must be done with its set
      if (k >= 2 && finishers[k - 2].joinable()) finishers[k - 2].join();
      H->pin = ctx->hsIn[k & 1].p; H->pinSlot = pslot;
    }
    kz_ctx* cx = ctx;
    finishers.emplace_back([H, cnt, k, trace, &ms, staged, cx]() {
      const double t0 = ms();
      if (staged) host_inverse_chunk_staged(cx, H, cnt, k & 1);
      else kz_parallel_for(cnt, KZ_HOST_STAGE_THREADS, host_inverse_block, H);
      if (trace) fprintf(stderr, "[pipe] decode chunk %d: host inverse stages %.0f .. %.0f ms\n", k, t0, ms());
    });
  }
  for (auto& t : finishers) if (t.joinable()) t.join();
  if (trace) fprintf(stderr, "[pipe] decode done at %.0f ms\n", ms());
  if (rc) { decode_error_sync(ctx); return rc; }
  for (int k = 0; k < nch; k++) {
    if (jobs[k]->fail) { snprintf(ctx->err, sizeof(ctx->err), "host stage: copy from / to the device failed"); return -KZ_ERR_DEVICE; }
    const int b0 = k * CH;
    for (size_t i = 0; i < lens[k].size(); i++) {
      kz_block_result& r = c.results[b0 + (int)i];
      if (!stats[k][i] && lens[k][i] > c.blockSize) stats[k][i] = -KZ_ERR_PROCESS_BLOCK;
      r.status = stats[k][i];
      r.length = stats[k][i] ? 0 : lens[k][i];
    }
  }
  return 0;
}
extern "C" int32_t kz_decode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                    const uint8_t* in, int64_t inStride, const int64_t* bitLengths, int32_t nBlocks,
                                    uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  if (nBlocks <= 0) return 0;
  // ---- the layout contract of include/kanzi_hip.h, checked on the whole batch before anything is copied or launched: a device
  //      slot is read in place, a few bytes ahead of the bit the decoder is at, so it carries KZ_STREAM_SLACK bytes behind its
  //      stream; a host stream is copied ((bits + 7) / 8 bytes) into a slot of the library's own ----
  if (!in || !out || !bitLengths || !results) { snprintf(ctx->err, sizeof(ctx->err), "decode: null pointer"); return -KZ_ERR_INVALID_PARAM; }
  for (int b = 0; b < nBlocks; b++) if (bitLengths[b] < 0) { snprintf(ctx->err, sizeof(ctx->err), "bitLengths[%d] < 0", b); return -KZ_ERR_INVALID_PARAM; }
  const DecodeCall c{entropyType, blockSize, in, inStride, bitLengths, nBlocks, out, outStride, results, memKind};
  Chain C;
  chain_split(transformType, C);                                    // (the plan reads the host prefix alone; the chain is checked below)
  const DecodePlan p = decode_plan(ctx, C, c, false);
  const int64_t needIn = p.maxInBytes + (memKind == KZ_MEM_DEVICE ? KZ_STREAM_SLACK : 0);
  if (inStride < needIn && (memKind == KZ_MEM_DEVICE || nBlocks > 1)) { snprintf(ctx->err, sizeof(ctx->err), "inStride %lld < %lld (longest stream%s)", (long long)inStride, (long long)needIn, memKind == KZ_MEM_DEVICE ? " + KZ_STREAM_SLACK" : ""); return -KZ_ERR_INVALID_PARAM; }
  if (outStride < 0) { snprintf(ctx->err, sizeof(ctx->err), "outStride %lld < 0", (long long)outStride); return -KZ_ERR_INVALID_PARAM; }
  int32_t rc = set_device(ctx);
  if (!rc) rc = chain_parse(ctx, transformType, entropyType, C);
  if (rc) { decode_error_sync(ctx); return rc; }
  // (block checksums are verified on the device AFTER the host stages: that case takes the one-pass path)
  if (C.hp > 0 && ctx->checksum == 0 && nBlocks >= 2 * ctx->sw.hostChunkDec && !p.textGpu) return decode_host_chunk_pipeline(ctx, C, c, p);
  rc = decode_blocks_impl(ctx, C, c, false);
  if (rc) decode_error_sync(ctx);
  return rc;
}
