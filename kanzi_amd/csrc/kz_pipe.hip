// kz_pipe.hip -- the codec tables, the parsed chain and the batch plumbing of the batched drivers (kz_pipe.h): the role of
// K/transform/Sequence.java's skip flags and pass-through.
#include "kz_pipe.h"
#include "kz_cm_host.h"
#include <stdlib.h>

// =================================================================================================
// ids / sizes
static int bwt_group_blocks(int B, int maxLen);
static int bwt_forward_grouped(kz_ctx* ctx, kz_batch& bt);
#define LEN(expr) [](int n) -> int { return expr; }
#define SCRATCH(expr) [](int B, int maxN, bool decode) -> size_t { return expr; }
#define STAGE(fn, ...) [](kz_ctx* ctx, kz_batch& bt, int dstCap, int entropy) -> int { return fn(ctx, bt, ##__VA_ARGS__); }   // fn(ctx, bt, the mode arguments)
#define TIMERS(X) KZ_STAGE_##X##_FWD, KZ_STAGE_##X##_INV
static const TransformRow kTransforms[] = {
  {KZ_T_NONE, LEN(n), nullptr, nullptr, nullptr, TIMERS(ZRLT)},   // NullTransform.java:107-109
  {KZ_T_TEXT, LEN(n), nullptr, nullptr, nullptr, TIMERS(ZRLT), true},   // TextCodec.java:1033-1037
  {KZ_T_UTF, LEN(n + 8192), nullptr, nullptr, nullptr, TIMERS(ZRLT), true},   // UTFCodec.java:308-310
  {KZ_T_BWT, LEN(n + 33), SCRATCH(decode ? kz_bwt_inverse_scratch(B, maxN) : kz_bwt_forward_scratch(bwt_group_blocks(B, maxN), maxN)),
   STAGE(bwt_forward_grouped), STAGE(kz_stage_bwt_inverse), TIMERS(BWT)},   // BWTBlockCodec.java:40,222
  {KZ_T_RANK, LEN(n), SCRATCH(kz_sbrt_scratch(B, maxN)), STAGE(kz_stage_sbrt_forward, 2), STAGE(kz_stage_sbrt_inverse, 2), TIMERS(SBRT)},   // SBRT.java:224
  {KZ_T_MTFT, LEN(n), SCRATCH(kz_sbrt_scratch(B, maxN)), STAGE(kz_stage_sbrt_forward, 1), STAGE(kz_stage_sbrt_inverse, 1), TIMERS(SBRT)},
  {KZ_T_ZRLT, LEN(n), SCRATCH(kz_zrlt_scratch(B, maxN)), STAGE(kz_stage_zrlt_forward), STAGE(kz_stage_zrlt_inverse, dstCap), TIMERS(ZRLT)},   // ZRLT.java:243
  {KZ_T_RLT, LEN((n <= 512) ? n + 32 : n), SCRATCH(kz_rlt_scratch(B, maxN) + (size_t)B * 4 + 256),   // RLT.java:419-421; + the per-block dst.length of the batched forward
   STAGE(kz_stage_rlt_forward, entropy), STAGE(kz_stage_rlt_inverse, dstCap), TIMERS(ZRLT)},
  {KZ_T_SRT, LEN(n + 1024), SCRATCH(decode ? 4096 : kz_srt_scratch(B, maxN)), STAGE(kz_stage_srt_forward), STAGE(kz_stage_srt_inverse), TIMERS(SRT)},   // SRT.java:30,365
  {KZ_T_LZ, LEN(((n <= 1024) ? n + 16 : n + (n / 64)) + 2), SCRATCH(decode ? 4096 : kz_lz_scratch(B, maxN)),   // LZCodec.java:961-964
   STAGE(kz_stage_lz_forward, 0), STAGE(kz_stage_lz_inverse, 0, dstCap), TIMERS(LZ)},
  {KZ_T_LZX, LEN(((n <= 1024) ? n + 16 : n + (n / 64)) + 2), SCRATCH(decode ? 4096 : kz_lz_scratch(B, maxN)),
   STAGE(kz_stage_lz_forward, 1), STAGE(kz_stage_lz_inverse, 1, dstCap), TIMERS(LZ)},
  {KZ_T_LZP, LEN((n <= 1024) ? n + 16 : n + (n / 64)), SCRATCH(kz_lzp_scratch(B, maxN)),   // LZCodec.java:1284-1286; the hash table, in both directions
   STAGE(kz_stage_lzp_forward), STAGE(kz_stage_lzp_inverse, dstCap), TIMERS(LZ)},
  {KZ_T_EXE, LEN((n <= 256) ? n + 32 : n + n / 8), SCRATCH(kz_exe_scratch(B, maxN, decode)),   // EXECodec.java:653-656
   STAGE(kz_stage_exe_forward), STAGE(kz_stage_exe_inverse, dstCap), TIMERS(ZRLT)},
  {KZ_T_MM, LEN(n + std::max(64, n >> 4)), SCRATCH(kz_mm_scratch(B, maxN)), STAGE(kz_stage_mm_forward), STAGE(kz_stage_mm_inverse, dstCap), TIMERS(ZRLT)},   // FSDCodec.java:323-325
  {KZ_T_PACK, LEN(n + 1024), SCRATCH(kz_alias_scratch(B, maxN, decode)),   // AliasCodec.java:445-447
   STAGE(kz_stage_alias_forward, 0), STAGE(kz_stage_alias_inverse, dstCap), TIMERS(ZRLT)},
  {KZ_T_DNA, LEN(n + 1024), SCRATCH(kz_alias_scratch(B, maxN, decode)),   // PACK with onlyDNA, TransformFactory.java:341-343
   STAGE(kz_stage_alias_forward, 1), STAGE(kz_stage_alias_inverse, dstCap), TIMERS(ZRLT)},
};
const TransformRow* transform_row(int t) { for (const TransformRow& r : kTransforms) if (r.id == t) return &r; return nullptr; }
bool host_stage(int t) { const TransformRow* r = transform_row(t); return r && r->host; }
extern "C" int32_t kz_transform_max_encoded_len(uint32_t type, int32_t n) { const TransformRow* r = transform_row((int)type); return r ? r->maxLen(n) : n; }
static int64_t ans1_max_stream_bytes(int n) { return (int64_t)kz_align((size_t)n + (size_t)(n >> 3) + 1024 + 102400 * ((size_t)n / (1 << 22) + 1), 256); }
static size_t ans0_scratch(int B, int maxN, bool decode) { return decode ? (size_t)B * ((size_t)(maxN / 16384 + 4) * 8 + 64) + 65536 : kz_ans_scratch(B, maxN); }   // and HUFFMAN: 16 KiB chunks
static const EntropyRow kEntropies[] = {
  {KZ_E_NONE, nullptr, nullptr, nullptr, kz_max_block_stream_bytes, nullptr, false, 0, true},
  {KZ_E_HUFFMAN, kz_stage_huffman_encode, kz_stage_huffman_decode, ans0_scratch, kz_max_block_stream_bytes, nullptr, false, 0, true},
  {KZ_E_FPAQ, kz_stage_fpaq_encode, kz_stage_fpaq_decode, SCRATCH(decode ? 4096 : kz_fpaq_scratch(B, maxN)), kz_max_block_stream_bytes, nullptr, true, 0, false},
  {KZ_E_RANGE, kz_stage_range_encode, kz_stage_range_decode, kz_range_scratch, kz_range_max_stream_bytes, "range encode: a chunk's payload does not fit its buffer", false, 0, true},
  {KZ_E_ANS0, kz_stage_ans0_encode, kz_stage_ans0_decode, ans0_scratch, kz_max_block_stream_bytes, nullptr, false, 0, true},
  {KZ_E_CM, kz_stage_cm_encode, kz_stage_cm_decode, kz_cm_scratch, kz_max_block_stream_bytes, "cm encode: the block's stream does not fit its buffer", true, KZ_CM_MAX_BLOCK, false},
  {KZ_E_ANS1, kz_stage_ans1_encode, kz_stage_ans1_decode, kz_ans1_scratch, ans1_max_stream_bytes, nullptr, false, 0, false},
};
const EntropyRow* entropy_row(uint32_t e) { for (const EntropyRow& r : kEntropies) if ((uint32_t)r.id == e) return &r; return nullptr; }
#undef LEN
#undef SCRATCH
#undef STAGE
#undef TIMERS
bool kz_fast_coder(int entropyType) { const EntropyRow* r = entropy_row((uint32_t)entropyType); return r && r->fast; }
extern "C" uint64_t kz_transform_type(const int32_t* types, int32_t nb) {   // TransformFactory.java:132-158
  uint64_t t = 0;
  for (int i = 0; i < 8; i++) t = (t << 6) | (uint64_t)((i < nb) ? (types[i] & 0x3F) : 0);
  return t;
}
static int split_types(uint64_t tt, int* types) {                    // TransformFactory.java:240-266
  int nbtr = 0;
  for (int i = 0; i < 8; i++) if (((tt >> (42 - 6 * i)) & 0x3F) != KZ_T_NONE) nbtr++;
  if (nbtr == 0) nbtr = 1;
  int k = 0;
  for (int i = 0; i < nbtr; i++) { int t = (int)((tt >> (42 - 6 * i)) & 0x3F); if (t != KZ_T_NONE || i == 0) types[k++] = t; }
  return k;
}
int seq_max_len(const int* types, int nb, int n) {             // Sequence.java:215-226
  int req = n;
  for (int i = 0; i < nb; i++) req = std::max(req, kz_transform_max_encoded_len((uint32_t)types[i], req));
  return req;
}
extern "C" int64_t kz_max_block_stream_bytes(int32_t n) { return (int64_t)kz_align((size_t)n + (size_t)(n >> 3) + 1024, 256); }
void chain_split(uint64_t transformType, Chain& C) {
  C.nb = split_types(transformType, C.types);
  C.hp = 0;
  while (C.hp < C.nb && host_stage(C.types[C.hp])) C.hp++;
}
int chain_parse(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, Chain& C) {
  chain_split(transformType, C);
  for (int i = 0; i < C.nb; i++) if (!transform_row(C.types[i])) { snprintf(ctx->err, sizeof(ctx->err), "unsupported transform id %d", C.types[i]); return -KZ_ERR_INVALID_CODEC; }
  C.E = entropy_row(entropyType); if (!C.E) { snprintf(ctx->err, sizeof(ctx->err), "unsupported entropy id %u", entropyType); return -KZ_ERR_INVALID_CODEC; }
  for (int i = C.hp; i < C.nb; i++)
    if (host_stage(C.types[i])) {
      snprintf(ctx->err, sizeof(ctx->err), "TEXT / UTF are built as host stages in front of the GPU stages only (as in the reference's levels)");
      return -KZ_ERR_INVALID_CODEC;
    }
  C.spec.nb = C.nb; C.spec.entropy = (int)entropyType; for (int i = 0; i < C.nb; i++) C.spec.types[i] = C.types[i];
  return 0;
}

// =================================================================================================
// small device helpers
__global__ void k_mask_len(const int32_t* __restrict__ len, const int32_t* __restrict__ mask, int32_t* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = mask[b] ? len[b] : 0;
}
// pass-through for blocks whose stage did not run (mask==0) or declined (flag==0)
__global__ void k_passthrough(const u8* __restrict__ src, u8* __restrict__ dst, int64_t stride, const int32_t* __restrict__ lenOld,
                              int32_t* __restrict__ lenNew, const int32_t* __restrict__ mask, const int32_t* __restrict__ flag,
                              int32_t* __restrict__ applied, const int32_t* __restrict__ part) {
  const int b = blockIdx.y;
  if (part && !part[b]) {                                           // not this pass's business: the slot is left alone
    if (blockIdx.x == 0 && threadIdx.x == 0) { applied[b] = 0; lenNew[b] = lenOld[b]; }
    return;
  }
  const bool ran = mask[b] != 0 && flag[b] > 0;                     // flag < 0: the reference's transform would have thrown
  if (blockIdx.x == 0 && threadIdx.x == 0) { applied[b] = ran ? 1 : ((mask[b] != 0 && flag[b] < 0) ? -1 : 0); if (!ran) lenNew[b] = lenOld[b]; }
  if (ran) return;
  const int n = lenOld[b];
  const u8* s = src + (int64_t)b * stride;
  u8* d = dst + (int64_t)b * stride;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n; i += gridDim.x * blockDim.x * 16) {
    if (i + 16 <= n) *(uint4*)(d + i) = *(const uint4*)(s + i);
    else for (int k = i; k < n; k++) d[k] = s[k];
  }
}
__global__ void k_copy_bytes(const u8* __restrict__ src, int64_t sstride, u8* __restrict__ dst, int64_t dstride,
                             const int32_t* __restrict__ len, const int32_t* __restrict__ dstOff, const int32_t* __restrict__ cond) {
  const int b = blockIdx.y;
  if (cond && !cond[b]) return;
  const int n = len[b];
  const u8* s = src + (int64_t)b * sstride;
  u8* d = dst + (int64_t)b * dstride + (dstOff ? dstOff[b] : 0);
  const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  if (((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {            // both 16-byte aligned (uniform per block): 16 bytes per lane
    const int n16 = n >> 4;
    for (int i = t; i < n16; i += nt) ((uint4*)d)[i] = ((const uint4*)s)[i];
    for (int i = (n16 << 4) + t; i < n; i += nt) d[i] = s[i];
  } else {
    for (int i = t; i < n; i += nt) d[i] = s[i];
  }
}

int sync_lengths(kz_ctx* ctx, kz_batch& bt) {
  KZ_HIP(hipMemcpyAsync(ctx->hpin, bt.d_len, (size_t)bt.B * 4, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  for (int b = 0; b < bt.B; b++) bt.h_len[b] = ctx->hpin[b];
  return 0;
}

int upload_mask(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask) {
  KZ_HIP(hipMemcpyAsync(P.d_mask, h_mask.data(), (size_t)P.bt.B * 4, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}
int mask_lengths(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask) {
  kz_batch& bt = P.bt;
  const int B = bt.B;
  const int rc = upload_mask(ctx, P, h_mask);
  if (rc) return rc;
  // save true lengths, run on masked lengths
  KZ_HIP(hipMemcpyAsync(P.d_lenSave, bt.d_len, (size_t)B * 4, hipMemcpyDeviceToDevice, ctx->stream));
  KZ_LAUNCH(ctx, KID_MASK_LEN, k_mask_len, dim3((B + 255) / 256), dim3(256), P.d_lenSave, P.d_mask, bt.d_len, B);
  return 0;
}
void pipe_copy_bytes(kz_ctx* ctx, int B, const u8* src, int64_t sstride, u8* dst, int64_t dstride, const int32_t* len, const int32_t* dstOff, const int32_t* cond) {
  KZ_LAUNCH(ctx, KID_COPY_BYTES, k_copy_bytes, dim3(64, B), dim3(256), src, sstride, dst, dstride, len, dstOff, cond);
}
void pipe_copy_bytes_on(hipStream_t s, int B, const u8* src, int64_t sstride, u8* dst, int64_t dstride, const int32_t* len, const int32_t* cond) {
  hipLaunchKernelGGL(k_copy_bytes, dim3(32, B), dim3(256), 0, s, src, sstride, dst, dstride, len, (const int32_t*)nullptr, cond);
}
int run_stage(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask, std::vector<int32_t>& h_applied, const std::function<int(kz_batch&)>& stage, const int32_t* d_part) {
  kz_batch& bt = P.bt;
  const int B = bt.B;
  hipStream_t st = ctx->stream;
  int rc = mask_lengths(ctx, P, h_mask);
  if (rc) return rc;
  for (int b = 0; b < B; b++) if (!h_mask[b]) bt.h_len[b] = 0;
  const u8* srcBefore = bt.buf[bt.cur];
  rc = stage(bt);
  if (rc) return rc;
  u8* dstAfter = bt.buf[bt.cur];
  KZ_LAUNCH(ctx, KID_PASSTHROUGH, k_passthrough, dim3(64, B), dim3(256), srcBefore, dstAfter, bt.stride, P.d_lenSave, bt.d_len, P.d_mask, bt.d_flag, P.d_applied, d_part);
  KZ_HIP(hipMemcpyAsync(ctx->hpin + B, P.d_applied, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  rc = sync_lengths(ctx, bt);
  if (rc) return rc;
  h_applied.resize(B);
  for (int b = 0; b < B; b++) h_applied[b] = ctx->hpin[B + b];
  return 0;
}

static size_t kz_arena_budget_probe() {
  const char* e = getenv("KZ_ARENA_BUDGET_GB");
  double gb = e ? atof(e) : 96.0;
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > 0) gb = std::min(gb, (double)freeB / (1 << 30) * 0.6);
  if (gb < 1.0) gb = 1.0;
  return (size_t)(gb * (double)(1 << 30));
}
size_t kz_arena_budget() {
  static const size_t budget = kz_arena_budget_probe();      // initialised once, also when contexts live on several threads
  return budget;
}
// stage scratch is bump-allocated after the ping-pong buffers; each stage allocates in turn, so the
// arena must hold the SUM over the stages the chain actually runs
// The forward BWT (suffix sort) needs ~43 B of scratch per input byte, an order of magnitude more than any
// other stage.  It therefore sorts the batch in groups that fit half the arena budget and reuses the scratch,
// while every other stage (and the serial-per-block entropy coders in particular) sees the whole batch.
static int bwt_group_blocks(int B, int maxLen) {
  const size_t per = kz_bwt_forward_scratch(1, maxLen);
  const int g = (int)std::max<size_t>(1, (kz_arena_budget() / 2) / per);
  if (g >= B) return B;
  const int groups = (B + g - 1) / g;                                // equal groups: 2 048 blocks at 341 per group used to end with a
  return (B + groups - 1) / groups;                                  // seventh group of TWO blocks paying every round's launches
}
size_t pipeline_scratch(int B, int maxLen, bool decode, const ChainSpec& C) {
  const EntropyRow* E = entropy_row((uint32_t)C.entropy);
  size_t s = 65536 + (E && E->scratch ? E->scratch(B, maxLen, decode) : 0);
  for (int i = 0; i < C.nb; i++) if (const TransformRow* r = transform_row(C.types[i])) if (r->scratch) s += r->scratch(B, maxLen, decode);
  return s;
}

int pipe_setup(kz_ctx* ctx, Pipe& P, int B, int maxLen, int64_t extraBytes, bool decode, const ChainSpec& C) {
  kz_batch& bt = P.bt;
  bt.B = B; bt.maxN = maxLen;
  bt.stride = (int64_t)kz_align((size_t)maxLen + 4096, 256);
  const size_t fixed = (size_t)bt.stride * B * 2 + (size_t)B * 4 * 16 + 65536 + (size_t)extraBytes;
  int rc = kz_arena_reserve(ctx, fixed + pipeline_scratch(B, maxLen, decode, C) + (1 << 20));
  if (rc) return rc;
  rc = kz_hpin_reserve(ctx, (size_t)B * 9 + 64);
  if (rc) return rc;
  bt.buf[0] = (u8*)kz_arena_alloc(ctx, (size_t)bt.stride * B);
  bt.buf[1] = (u8*)kz_arena_alloc(ctx, (size_t)bt.stride * B);
  bt.d_len = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  bt.d_len2 = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  bt.d_flag = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  bt.d_dtype = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  P.d_mask = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  P.d_applied = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  P.d_lenSave = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  bt.cur = 0;
  bt.h_len.assign(B, 0);
  if (!P.d_lenSave || !bt.d_dtype) { snprintf(ctx->err, sizeof(ctx->err), "pipe_setup: arena overflow"); return -KZ_ERR_DEVICE; }
  KZ_HIP(hipMemsetAsync(bt.d_dtype, 0, (size_t)B * 4, ctx->stream));      // Global.DataType.UNDEFINED
  return 0;
}

static int bwt_forward_grouped(kz_ctx* ctx, kz_batch& bt) {
  const int B = bt.B;
  const int G = bwt_group_blocks(B, bt.maxN);
  if (G >= B) return kz_stage_bwt_forward(ctx, bt);
  const size_t mark = ctx->arenaTop;
  for (int b0 = 0; b0 < B; b0 += G) {
    const int cnt = std::min(G, B - b0);
    kz_batch v;                                   // a view of blocks [b0, b0+cnt)
    v.B = cnt; v.maxN = bt.maxN; v.stride = bt.stride; v.cur = bt.cur;
    v.buf[0] = bt.buf[0] + (int64_t)b0 * bt.stride; v.buf[1] = bt.buf[1] + (int64_t)b0 * bt.stride;
    v.d_len = bt.d_len + b0; v.d_len2 = bt.d_len2 + b0; v.d_flag = bt.d_flag + b0;
    v.h_len.assign(bt.h_len.begin() + b0, bt.h_len.begin() + b0 + cnt);
    ctx->arenaTop = mark;                         // the groups run back to back on one stream: reuse the scratch
    const int rc = kz_stage_bwt_forward(ctx, v);
    if (rc) return rc;
  }
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}

int run_transform_stage(kz_ctx* ctx, kz_batch& bt, int type, bool forward, int dstCap, int entropy) {
  const TransformRow* r = transform_row(type);
  if (!r || !r->forward) { snprintf(ctx->err, sizeof(ctx->err), "transform %d has no HIP stage", type); return -KZ_ERR_INVALID_CODEC; }
  return (forward ? r->forward : r->inverse)(ctx, bt, dstCap, entropy);
}
int stage_id(int type, bool forward) {                       // an id without a row: NONE's timers
  const TransformRow* r = transform_row(type) ? transform_row(type) : kTransforms; return forward ? r->timerFwd : r->timerInv; }
