// kz_pipe.h -- what the batched drivers share (internal): the codec tables, a parsed chain, the batch plumbing (kz_pipe.hip), the
// host TEXT / UTF stages (kz_host_stages.hip) and the decoder's overlap planner (kz_overlap.hip).  Users: kz_encode.hip,
// kz_decode.hip and the single-block calls of kz_api.hip.
#pragma once
#include "kz_device.h"
#include "kz_internal.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>

#pragma GCC visibility push(hidden)   // internal to the library: not part of its exported symbols
typedef uint32_t u32;
typedef uint8_t u8;
typedef unsigned long long u64;

// host threads of the TEXT / UTF stages.  The reference caps its jobs at 64 (BlockCompressor.java:199-203) on hosts of a few
// dozen cores; a GPU box brings hundreds, and these stages are what the GPU waits for in the level-exact chains: up to 128
// (every thread keeps a dictionary, stage buffers and a small alias map: a few MiB)
#define KZ_HOST_STAGE_THREADS 128

// ---- the codec tables (kz_pipe.hip): what the drivers know about a transform or an entropy coder is ONE row; a new stage adds a row
struct TransformRow {
  int id;                                             // KZ_T_*
  int (*maxLen)(int n);                               // ByteTransform.getMaxEncodedLength
  size_t (*scratch)(int B, int maxN, bool decode);    // arena bytes of the stage (null: none)
  int (*forward)(kz_ctx*, kz_batch&, int dstCap, int entropy);   // null: no device entry point (NONE, the host stages)
  int (*inverse)(kz_ctx*, kz_batch&, int dstCap, int entropy);
  int timerFwd, timerInv;                             // KZ_STAGE_*; a stage without a timer of its own is counted under ZRLT's
  bool host;                                          // TEXT, UTF: host stages; kz_is_host_transform (kz_text.hip, for the context-free kz_host_stage_* calls) names the same ids
};
struct EntropyRow {
  int id;                                             // KZ_E_*
  int (*encode)(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);   // null: NONE, the bytes as they are
  int (*decode)(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
  size_t (*scratch)(int B, int maxN, bool decode);    // arena bytes of the stage (null: none)
  int64_t (*streamBytes)(int n);                      // bound of a single block's stream (kz_entropy_encode's buffer)
  const char* overflow;                               // set: the encoder writes d_flag[b] = 0 for a block that outgrew its buffer, which fails; the text is kz_entropy_encode's
  bool flushEmpty;                                    // encode + dispose of an empty input still writes the 56-bit flush
  int blockLimit;                                     // blocks of this many bytes and more are refused (0: no limit; CM alone has one, and the two error texts beside the checks are CM's)
  bool fast;                                          // the reference's fast coders: TextCodec2, no escape search in RLT (TransformFactory.java:275-286, RLT.java:101-108)
};
const TransformRow* transform_row(int t);
const EntropyRow* entropy_row(uint32_t e);
bool host_stage(int t);
int seq_max_len(const int* types, int nb, int n);     // Sequence.java:215-226
int stage_id(int type, bool forward);
int run_transform_stage(kz_ctx* ctx, kz_batch& bt, int type, bool forward, int dstCap, int entropy);

// ---- a chain, parsed once per call
struct ChainSpec { int types[8]; int nb; int entropy; };
struct Chain { int types[8]; int nb; int hp; const EntropyRow* E; ChainSpec spec; };   // hp: the leading host stages (TEXT, UTF)
void chain_split(uint64_t transformType, Chain& C);   // types, nb and hp alone: no check, no error text (callers off the context's thread)
int chain_parse(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, Chain& C);   // the split, both "unsupported id" checks, no host stage behind a GPU stage

// ---- batch plumbing
struct Pipe {
  kz_batch bt;
  int32_t* d_mask = nullptr;      // [B] stage applies to this block
  int32_t* d_applied = nullptr;   // [B]
  int32_t* d_lenSave = nullptr;   // [B]
  int32_t* d_one = nullptr;       // [B] all ones
};
template <typename T> static inline T* kz_arena_array(kz_ctx* ctx, size_t n) { return (T*)kz_arena_alloc(ctx, n * sizeof(T)); }
int sync_lengths(kz_ctx* ctx, kz_batch& bt);
int upload_mask(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask);   // h_mask -> P.d_mask on the main stream (the caller syncs before h_mask goes away)
int mask_lengths(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask);  // upload_mask, d_len saved to P.d_lenSave, d_len = 0 where the mask is 0
// run one stage on the blocks selected by h_mask; others (and blocks where the transform declines)
// pass through unchanged.  On return h_applied[b] tells which blocks the transform was applied to.
int run_stage(kz_ctx* ctx, Pipe& P, const std::vector<int32_t>& h_mask, std::vector<int32_t>& h_applied, const std::function<int(kz_batch&)>& stage,
              const int32_t* d_part = nullptr);
size_t kz_arena_budget();
size_t pipeline_scratch(int B, int maxLen, bool decode, const ChainSpec& C);
int pipe_setup(kz_ctx* ctx, Pipe& P, int B, int maxLen, int64_t extraBytes, bool decode, const ChainSpec& C);
// k_copy_bytes (kz_pipe.hip) for the other files: over B blocks on the main stream (timed), or on a stream of the caller's
void pipe_copy_bytes(kz_ctx* ctx, int B, const u8* src, int64_t sstride, u8* dst, int64_t dstride, const int32_t* len, const int32_t* dstOff, const int32_t* cond);
void pipe_copy_bytes_on(hipStream_t s, int B, const u8* src, int64_t sstride, u8* dst, int64_t dstride, const int32_t* len, const int32_t* cond);

__device__ __forceinline__ u32 kz_mix32(u32 c, u32 h, u32 v) {        // CompressedOutputStream.java:89-93
  c ^= h * ~v;
  c = (c << 13) | (c >> 19);
  return c * 5u + 0x52DCE729u;
}
__device__ __forceinline__ u8 kz_block_cksum(u32 mode, u32 hsf, u32 postLen, u64 written) {   // :977-985
  const u32 HASH = 0x1E35A7BDu;
  u32 c = HASH * 0x01030507u;
  c = kz_mix32(c, HASH, mode);
  c = kz_mix32(c, HASH, hsf);
  c = kz_mix32(c, HASH, postLen);
  c = kz_mix32(c, HASH, (u32)(written >> 32));
  c = kz_mix32(c, HASH, (u32)written);
  c = (c >> 23) ^ (c >> 3);
  return (u8)c;
}

// ---- host (CPU) stages (kz_host_stages.hip)
// Result of the host stages (TEXT, UTF) of a set of blocks, computed host -> host so that it can run on a helper thread while the
// GPU codes the previous set: per block its length, skip flag bits and "dataType" entry, and -- when a stage applied -- the
// transformed bytes (slot b of `store`).
struct HostPre {
  std::vector<int32_t> outLen, skip, dtype;
  std::vector<uint8_t> changed;
  std::unique_ptr<uint8_t[]> own;                   // the slots' memory when the caller gave none
  uint8_t* store = nullptr;
  bool pinned = false;                              // store is pinned host memory (a kernel can read it: one gather instead of a copy per block)
  int64_t slot = 0;
  const uint8_t* data(int b) const { return store + (int64_t)b * slot; }
  HostPre view(int b0, int cnt) const;              // blocks [b0, b0 + cnt): the slots stay where they are
};
int64_t host_pre_slot(int cap);
// store: B slots of host_pre_slot(cap) bytes for the stages' outputs (pinned staging of the pipelines), or null
void host_prestage(const Chain& C, int blockSize, int cap, const uint8_t* hsrc, int64_t hstride, const int32_t* lengths, const int32_t* copy, int B,
                   HostPre& P, uint8_t* store = nullptr);
// the same over a list of blocks (block k at ptrs[k], lengths[k] bytes): the results are numbered like the list
// store: K slots of host_pre_slot(cap) bytes (pinned: the per-block copies back to HBM are then real DMA), or null
void host_prestage_list(const Chain& C, int blockSize, int cap, const std::vector<const uint8_t*>& ptrs, const std::vector<int32_t>& lengths, HostPre& P,
                        uint8_t* store = nullptr, const std::vector<int32_t>* first = nullptr, const std::vector<int32_t>* dt0 = nullptr);
struct HostInv {
  int device; const int* types; int hp; int blockSize; int cap;
  uint8_t* dbuf; int64_t dstride; int64_t slotCap; bool hostMem;        // the blocks' slots: in HBM (copied over and back) or in host memory
  int32_t* len; const int32_t* skip; int32_t* status; std::atomic<int> fail{0};
  uint8_t* pin = nullptr; int64_t pinSlot = 0;                          // staged form: the chunk's blocks were gathered into pinned slots
};
// the host inverse stages of blocks in slots `stride` apart, of capacity `stride` each
void host_inv_make(HostInv& H, const kz_ctx* ctx, const Chain& C, int blockSize, int cap, uint8_t* slots, int64_t stride, bool hostMem, int32_t* len,
                   const int32_t* skip, int32_t* status);
void host_inverse_block(int b, void* arg);            // arg: a HostInv
void host_inverse_chunk_staged(kz_ctx* ctx, HostInv* H, int cnt, int ring);

// ---- the decoder's overlapped RANK / BWT inverse and the device-stage predicates (kz_overlap.hip)
int text_gpu_form(const kz_ctx* ctx, uint32_t entropyType, int nBlocks);
inline bool text_gpu_on(const kz_ctx* ctx, uint32_t entropyType, int nBlocks) { return text_gpu_form(ctx, entropyType, nBlocks) != 0; }
// UTF inverse on the device (kz_text_gpu.hip: parallel inside a block, so for any batch); KZ_UTF_GPU=0 keeps it on the host
inline bool utf_gpu_on(const kz_ctx* ctx) { return ctx->sw.utfGpu != 0; }
// One cost class of the batch: a lengths-masked view of the same slots with its own length / flag arrays.
struct OverlapGroup {
  std::vector<int32_t> in;
  int32_t *d_in = nullptr, *len = nullptr, *len2 = nullptr, *flag = nullptr, *old = nullptr;
  int prio = 0;
  int ev = -1;                            // index of the side stream / join event of its RANK inverse (-1: on the main stream)
  double tPre = 0, tRank = 0, tBwt = 0;   // modelled seconds of the group's entropy + ZRLT pass, RANK inverse and BWT inverse
  kz_batch v;
};
// groups[0] goes on the main stream (the cheapest class), groups[1..] on the side streams, most expensive last
struct Overlap { std::vector<OverlapGroup> groups; std::vector<int> launchOrder, bwtOrder; int mainGroup = -1; int64_t started = 0;
                 std::vector<std::vector<int>> bwtCalls; };   // bwtCalls: the groups of bwtOrder whose BWT inverses run as ONE call (empty: one call per group)
bool overlap_classify(const kz_ctx* ctx, int B, const std::vector<int32_t>& h_mask, const std::vector<int32_t>& cost, Overlap& O);
int overlap_alloc(kz_ctx* ctx, int B, Overlap& O);
void overlap_plan(kz_ctx* ctx, Overlap& O, const std::vector<int32_t>& zlen, const std::vector<int32_t>& rawp, int blockSize, bool withPre);
int overlap_start_rank(kz_ctx* ctx, const kz_batch& bt, int mode, Overlap& O, int g, int k);
int overlap_finish(kz_ctx* ctx, Pipe& P, Overlap& O, std::vector<int32_t>& h_applied);
int overlapped_rank_bwt_inverse(kz_ctx* ctx, Pipe& P, int mode, const std::vector<int32_t>& h_mask, const std::vector<int32_t>& cost, std::vector<int32_t>& h_applied);

// ---- kz_encode.hip, for the job queue of kz_api.hip
int32_t encode_block_size(kz_ctx* ctx, uint64_t transformType);
#pragma GCC visibility pop
