// kz_internal.h -- host-side context + stage interfaces (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <mutex>
#include <thread>
#include "../../include/kanzi_hip.h"

// every kernel once, in the order of its id: KzKernelId and the names that bench.py and tools/pmc_traffic.py key on come from this list
#define KZ_KERNELS(X) \
  X(KID_ANS_ENC_CHUNK, "k_ans_enc_chunk") X(KID_ANS_ENC_SCAN, "k_ans_enc_scan") X(KID_ANS_ENC_CONCAT, "k_ans_enc_concat") X(KID_ANS_DEC_INDEX, "k_ans_dec_index") \
  X(KID_ANS_DEC_CHUNK, "k_ans_dec_chunk") X(KID_ANS_DEC_FIN, "k_ans_dec_fin") X(KID_MASK_LEN, "k_mask_len") X(KID_PASSTHROUGH, "k_passthrough") \
  X(KID_FRAME_PREPARE, "k_frame_prepare") X(KID_COPY_BYTES, "k_copy_bytes") X(KID_FRAME_DECIDE, "k_frame_decide") X(KID_FRAME_HEADER, "k_frame_header") \
  X(KID_FRAME_PARSE, "k_frame_parse") X(KID_COPY_PAYLOAD, "k_copy_payload") X(KID_BWT_INIT, "k_bwt_init") X(KID_RADIX_HIST, "k_radix_hist") \
  X(KID_RADIX_SCAN, "k_radix_scan") X(KID_RADIX_SCATTER, "k_radix_scatter") X(KID_SEG_REDUCE, "k_seg_reduce") X(KID_SEG_SCAN, "k_seg_scan") \
  X(KID_SEG_APPLY, "k_seg_apply") X(KID_LIVE_EMIT, "k_live_emit") X(KID_BWT_EMIT, "k_bwt_emit") X(KID_BWTI_PARSE, "k_bwti_parse") \
  X(KID_BWTI_HIST, "k_bwti_hist") X(KID_BWTI_SCAN, "k_bwti_scan") X(KID_BWTI_SCATTER, "k_bwti_scatter") X(KID_BWTI_WALK1, "k_bwti_walk1") \
  X(KID_BWTI_RESOLVE, "k_bwti_resolve") X(KID_BWTI_COPY, "k_bwti_copy") X(KID_BWTI_LITERAL, "k_bwti_literal") X(KID_BWTI_FIN, "k_bwti_fin") \
  X(KID_SBRT_LAST2, "k_sbrt_last2") X(KID_SBRT_SCAN, "k_sbrt_scan") X(KID_SBRT_REPLAY, "k_sbrt_replay") X(KID_COPY_LEN, "k_copy_len") \
  X(KID_SBRT_INVERSE, "k_sbrt_inverse") X(KID_ZRLT_F1, "k_zrlt_f1") X(KID_ZRLT_F2, "k_zrlt_f2") X(KID_ZRLT_F3, "k_zrlt_f3") \
  X(KID_ZRLT_FFIN, "k_zrlt_ffin") X(KID_ZRLT_I1, "k_zrlt_i1") X(KID_ZRLT_I2, "k_zrlt_i2") X(KID_ZRLT_I3, "k_zrlt_i3") \
  X(KID_ZRLT_IFIN, "k_zrlt_ifin") X(KID_RLT_F0, "k_rlt_f0") X(KID_RLT_FSCAN, "k_rlt_fscan") X(KID_RLT_F1, "k_rlt_f1") \
  X(KID_RLT_FSUM, "k_rlt_fsum") X(KID_RLT_F3, "k_rlt_f3") X(KID_RLT_FTAIL, "k_rlt_ftail") X(KID_RLT_I1, "k_rlt_i1") \
  X(KID_RLT_ISCAN, "k_rlt_iscan") X(KID_RLT_I2, "k_rlt_i2") X(KID_RLT_ISUM, "k_rlt_isum") X(KID_RLT_I3, "k_rlt_i3") \
  X(KID_RLT_IFIN, "k_rlt_ifin") X(KID_HUF_ENC_CHUNK, "k_huf_enc_chunk") X(KID_HUF_DEC_INDEX, "k_huf_dec_index") X(KID_HUF_DEC_CHUNK, "k_huf_dec_chunk") \
  X(KID_HUF_DEC_FIN, "k_huf_dec_fin") X(KID_FPAQ_ENC, "k_fpaq_enc") X(KID_FPAQ_PACK, "k_fpaq_pack") X(KID_FPAQ_DEC, "k_fpaq_dec") \
  X(KID_SRT_HIST, "k_srt_hist") X(KID_SRT_PREP, "k_srt_prep") X(KID_SRT_SCATTER, "k_srt_scatter") X(KID_SRT_INV, "k_srt_inv") \
  X(KID_LZ_FWD, "k_lz_fwd") X(KID_LZ_INV, "k_lz_inv") X(KID_XXHASH, "k_xxhash") X(KID_BLOCK_MAGIC, "k_block_magic") \
  X(KID_MM_ANALYZE, "k_mm_analyze") X(KID_MM_EMIT, "k_mm_emit") X(KID_MM_CHECK, "k_mm_check") X(KID_MM_INV, "k_mm_inv") \
  X(KID_ALIAS_ANALYZE, "k_alias_analyze") X(KID_ALIAS_HIST1, "k_alias_hist1") X(KID_ALIAS_SELECT, "k_alias_select") X(KID_ALIAS_EMIT, "k_alias_emit") \
  X(KID_ALIAS_INV, "k_alias_inv") X(KID_SKIP_DECIDE, "k_skip_decide") X(KID_MSD_HIST, "k_msd_hist") X(KID_MSD_SCAN, "k_msd_scan") \
  X(KID_MSD_SCATTER, "k_msd_scatter") X(KID_BUCKET_SORT, "k_bucket_sort") X(KID_BUCKET_COUNT, "k_bucket_count") X(KID_BUCKET_COUNT_S, "k_bucket_count_s") \
  X(KID_TR_HIST16, "k_tr_hist16") X(KID_TR_ASSIGN, "k_tr_assign") X(KID_TR_COUNT, "k_tr_count") X(KID_TR_SCATTER, "k_tr_scatter") \
  X(KID_TR_SORT, "k_tr_sort") X(KID_TEXT_INV, "k_text_inv") X(KID_UTF_INV, "k_utf_inv") X(KID_TEXT_FWD, "k_text_fwd") \
  X(KID_TEXT_WALK, "k_text_walk") X(KID_UTF_FWD, "k_utf_fwd") X(KID_ANS1_HIST, "k_ans1_hist") X(KID_ANS1_NORM, "k_ans1_norm") \
  X(KID_ANS1_HDR, "k_ans1_hdr") X(KID_ANS1_ENC, "k_ans1_enc") X(KID_ANS1_DEC_INDEX, "k_ans1_dec_index") X(KID_ANS1_DEC_TABLE, "k_ans1_dec_table") \
  X(KID_ANS1_DEC_CHUNK, "k_ans1_dec_chunk") X(KID_ANS1_DEC_FIN, "k_ans1_dec_fin") X(KID_RANGE_ENC_CHUNK, "k_range_enc_chunk") X(KID_RANGE_ENC_FIN, "k_range_enc_fin") \
  X(KID_RANGE_DEC, "k_range_dec") X(KID_CM_ENC, "k_cm_enc") X(KID_CM_DEC, "k_cm_dec") X(KID_LZP_FWD, "k_lzp_fwd") \
  X(KID_LZP_INV, "k_lzp_inv") X(KID_EXE_SETUP, "k_exe_setup") X(KID_EXE_MAP, "k_exe_map") X(KID_EXE_SCAN, "k_exe_scan") \
  X(KID_EXE_HIST, "k_exe_hist") X(KID_EXE_DECIDE, "k_exe_decide") X(KID_EXE_SIZE, "k_exe_size") X(KID_EXE_VERDICT, "k_exe_verdict") \
  X(KID_EXE_EMIT, "k_exe_emit") X(KID_KNZ_PACK, "k_knz_pack") X(KID_KNZ_WALK, "k_knz_walk") X(KID_KNZ_UNPACK, "k_knz_unpack") \
  X(KID_KNZ_CHECK, "k_knz_check") X(KID_KNZ_GATHER, "k_knz_gather") X(KID_KNZ_PACK_MANY, "k_knz_pack_many") X(KID_KNZ_HEADS, "k_knz_heads") \
  X(KID_KNZ_WALK_MANY, "k_knz_walk_many") X(KID_KNZ_UNPACK_MANY, "k_knz_unpack_many") X(KID_KNZ_SCATTER, "k_knz_scatter") \
  X(KID_KNZ_CHECK_MANY, "k_knz_check_many") X(KID_KNZ_SPLICE, "k_knz_splice") X(KID_KNZ_READ, "k_knz_read") X(KID_KNZ_WRITE, "k_knz_write") \
  X(KID_KNZ_SCAN_COUNT, "k_knz_scan_count") X(KID_KNZ_SCAN_SUM, "k_knz_scan_sum") X(KID_KNZ_SCAN_WRITE, "k_knz_scan_write") X(KID_KNZ_SCAN_LINK, "k_knz_scan_link") \
  X(KID_KNZ_SCAN_RUN, "k_knz_scan_run") X(KID_KNZ_SCAN_MARK, "k_knz_scan_mark") X(KID_KNZ_SCAN_EMIT, "k_knz_scan_emit") X(KID_KNZ_CHECK_ROWS, "k_knz_check_rows") \
  X(KID_KNZ_SPLICE_MANY, "k_knz_splice_many")
#define KZ_KERNEL_ENUM(id, name) id,
#define KZ_KERNEL_NAME(id, name) name,
enum KzKernelId { KZ_KERNELS(KZ_KERNEL_ENUM) KID_COUNT };
#define KZ_KERNEL_NAMES { KZ_KERNELS(KZ_KERNEL_NAME) }
// Environment switches (diagnostics, A/B runs, the tests' forced schedules; none is needed for normal use).  Read ONCE, when the
// context is created (kz_switches_read, kz_api.hip); kz_ctx_reload_switches re-reads them for a live context (tests, A/B tools).
// Nothing on a call's path calls getenv.
struct kz_switches {
  int blockingWaits = -1;        // KZ_BLOCKING_WAITS: -1 unset (decided from the CPU quota), 0 / 1
  int textGpu = -1;              // KZ_TEXT_GPU: -1 unset, 0 host, 1 rows x 3 waves, 2 serial walk, 3 rows x 1 wave
  int textGpuMin = 512;          // KZ_TEXT_GPU_MIN
  int textFwdGpu = -1;           // KZ_TEXT_FWD_GPU: -1 unset, 0 host, 1 any batch
  int textFwdGpuMin = 256;       // KZ_TEXT_FWD_GPU_MIN
  int text1FwdGpu = -1;          // KZ_TEXT1_FWD_GPU: the same for TextCodec1 streams (FPAQ / CM / ANS1): -1 unset, 0 host, 1 any batch
  int text1FwdGpuMin = 64;       // KZ_TEXT1_FWD_GPU_MIN: batch size from which the unset case uses the device (0 = never; the default: kz_overlap.hip, text_fwd_gpu_on)
  int utfGpu = 1;                // KZ_UTF_GPU=0: UTF inverse on the host
  int utfFwdGpu = -1;            // KZ_UTF_FWD_GPU: -1 unset (with the device TEXT forward), 0 host, 1 any batch
  int textGpuTrace = 0;          // KZ_TEXT_GPU_TRACE
  int fuseMinBlocks = 32;        // KZ_FUSE_MIN_BLOCKS: smaller batches run the decoder's stages one after the other
  int overlapClasses = 3;        // KZ_OVERLAP_CLASSES
  int wideQueues = -1;           // KZ_WIDE_QUEUES: -1 = measured once per context
  int noSFirst = 0;              // KZ_NO_SFIRST
  int traceSched = 0;            // KZ_TRACE_SCHED
  int tracePipe = 0;             // KZ_TRACE_PIPE
  int hostChunk = 0;             // KZ_HOST_CHUNK (0: by the batch)
  int hostChunkDec = 512;        // KZ_HOST_CHUNK_DEC
  int hostInvStaged = -1;        // KZ_HOST_INV_STAGED: -1 unset
  int streamChunk = 0;           // KZ_STREAM_CHUNK (0: default)
  int streamSerial = 0;          // KZ_STREAM_SERIAL
  int readScatter = 0;           // KZ_READ_SCATTER: kz_read_bytes_device copies its segments with k_knz_scatter (tools/knz_read_probe.py's yardstick)
  int writeGather = 0;           // KZ_WRITE_GATHER: kz_write_bytes_device patches its rows with k_knz_gather (tools/knz_write_probe.py's yardstick)
  int bwtTrie = -1, bwtTrieWin = -1, bwtBuckets = -1, bwtDmax = -1, bwtRetire = -1;   // KZ_BWT_TRIE / _TRIEWIN / _BUCKETS / _DMAX / _RETIRE (-1 unset)
  int bwtLazyRank = -1;         // KZ_BWT_LAZYRANK=0: round 0 stores every rank (A/B; see k_tr_sort)
  int bwtLivePart = -1;          // KZ_BWT_LIVEPART=0: the bucket rounds partition the text-order list (k_live_emit, k_msd_hist, k_msd_scatter: A/B);
                                 // unset / 1: straight from the ranks (k_live_hist, k_live_scatter); N >= 2: only while the longest list is above maxN / N
  int bwtTrace = 0;              // KZ_BWT_TRACE
  int bwtTestTrieOverflow = -1;  // KZ_BWT_TEST_TRIE_OVERFLOW=<round> (tests)
  int fpaqForce = 0;             // KZ_FPAQ_FORCE: 0 unset, 1 wave, 2 lane
  int cmTestRowBytes = 0;        // KZ_CM_TEST_ROW_BYTES=<bytes> (tests): the CM encoder takes its output rows to be this short
  int sbrtForm = -1;             // KZ_SBRT_FORM: -1 default, 0 = the 32-bit list forms of rounds 2-5 (A/B)
};
void kz_switches_read(kz_switches& s);   // kz_api.hip

struct KzPending { hipEvent_t e0, e1; int id; };
struct kz_ctx {
  int device = 0;
  kz_switches sw;                // environment switches as read at creation
  hipStream_t stream = nullptr;
  hipStream_t side[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // side streams of the overlapped RANK-inverse / BWT-inverse schedule (created on first use)
  hipEvent_t evJoin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int wideQueues = -1;           // main + three side streams run side by side (-1: not measured yet)
  int wideNow = 0;               // what the current call uses (sw.wideQueues overrides the measurement)
  // grow-only device arena, bump-allocated per API call
  uint8_t* arena = nullptr;
  size_t arenaCap = 0, arenaTop = 0;
  // pinned host staging for small read-backs
  int32_t* hpin = nullptr;       // hpinInts ints, grown by kz_hpin_reserve
  size_t hpinInts = 0;
  char err[512] = {0};
  // last-call stage timings (ms) for bench/roofline (hipEvent based)
  float stageMs[KZ_MAX_STAGES] = {0};
  int64_t stageAlgBytes[KZ_MAX_STAGES] = {0};
  int nStages = 0;
  int checksum = 0;              // 0 none, 1 XXHash32, 2 XXHash64 (ctx map key "checksum")
  int skipBlocks = 0;            // ctx map key "skipBlocks": store incompressible-looking blocks as copy blocks
  int dataType = 0;              // ctx map key "dataType" for the single-block calls (Global.DataType, KZ_DT_*)
  int blockSize = 4 * 1024 * 1024;   // ctx map key "blockSize" (TEXT sizes its hash map by it)
  bool blockSizeSet = false;     // kz_ctx_set_block_size was called: chains with TEXT refuse to guess
  int entropy = KZ_E_NONE;       // ctx map key "entropy" for the single-block calls (TEXT: TextCodec1 / TextCodec2)
  int rltBlockSize = 0;          // the block size RLT's dst.length rule goes by, fixed by the outermost batched encode call (0: none running)
  int numCUs = 256;              // compute units of the device (placement of the serial-per-block kernels)
  long long* d_endBits = nullptr; // optional [B] device array: bit position behind each block's entropy payload (kz_entropy_decode)
  bool timing = false;
  // per-kernel event timing (bench roofline): events recorded on ctx->stream around every launch
  bool ktiming = false;
  std::vector<KzPending> pending;
  std::vector<hipEvent_t> evPool;
  double kMs[KID_COUNT] = {0};
  double kMaxMs[KID_COUNT] = {0};     // longest single launch (launches of one kernel on several streams overlap)
  long long kLaunches[KID_COUNT] = {0};
  // asynchronous batches (kz_submit_* / kz_wait): one worker thread per context runs the queued calls in order
  std::thread worker;
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<std::pair<int64_t, std::function<int32_t()>>> queue;
  std::map<int64_t, int32_t> finished;
  std::set<int64_t> collected;   // ids kz_wait has handed out (>= collectedBelow; everything below is collected too)
  int64_t collectedBelow = 1;
  int64_t nextJob = 1;
  bool stopWorker = false;
  // staging of the host-buffer stream calls (kz_compress / kz_decompress, kz_stream.hip): grow-only, two slots each
  struct Stage { uint8_t* p = nullptr; size_t cap = 0; };
  Stage pinIn[2], pinOut[2];       // pinned host memory (hipHostMalloc)
  Stage devIn[2], devOut[2];       // HBM outside the arena (the arena is reset by every batched call)
  Stage hsIn[2], hsOut[2];         // pinned: the host-stage pipeline's copy of a chunk's blocks / the stages' outputs (kz_encode.hip, kz_decode.hip)
  Stage tfIn, tfOut[2];           // pinned: the device TEXT forward's host passes (kz_encode_blocks_pre).  Their own buffers and
  hipStream_t tfCopy = nullptr;    // stream: kz_compress's upload thread fills hsOut[k & 1] / drains on copyDown for the NEXT chunk meanwhile
  hipStream_t copyUp = nullptr, copyDown = nullptr;
  Stage hiAux[2];                  // HBM: per-block lengths / masks of the decoder's host-inverse chunks (kz_decode.hip, kz_host_stages.hip)
  hipStream_t hiStream[2] = {nullptr, nullptr};   // their gather / scatter kernels run beside the main stream's next chunk
  Stage knzPin, knzAux;            // pinned / HBM: the device stream calls' per-chunk tables (bit offsets, lengths, header bytes; kz_stream_device.hip)
  // waits of the context's own thread: 1 = block on an event (hipEventBlockingSync) instead of hipStreamSynchronize's spin loop.
  // Chosen at creation: on when the process is CPU-quota limited (a spinning waiter burns a whole CPU of the quota that the
  // host stages -- or the other ranks of the node -- could use), KZ_BLOCKING_WAITS=0/1 overrides.
  int blockingWaits = 0;
  hipEvent_t evBlock = nullptr;
};

// scratch taken from the context's arena inside one function: given back on every way out (KZ_HIP returns early)
struct kz_arena_guard { kz_ctx* c; size_t mark; ~kz_arena_guard() { c->arenaTop = mark; } };

#define KZ_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  snprintf(ctx->err, sizeof(ctx->err), "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  return -KZ_ERR_DEVICE; } } while (0)

// wait for everything queued on `st` (the context's thread only)
static inline hipError_t kz_stream_sync(kz_ctx* ctx, hipStream_t st) {
  if (!ctx->blockingWaits) return hipStreamSynchronize(st);
  if (!ctx->evBlock) { hipError_t e = hipEventCreateWithFlags(&ctx->evBlock, hipEventBlockingSync | hipEventDisableTiming); if (e != hipSuccess) return e; }
  hipError_t e = hipEventRecord(ctx->evBlock, st);
  if (e != hipSuccess) return e;
  return hipEventSynchronize(ctx->evBlock);
}

#define KZ_MAX_PACKED_BLOCK ((1 << 24) - 257)   // largest block the packed inverse BWT / RANK kernels take (longer ones: their wide forms)
#define KZ_MAX_BLOCK ((1 << 30) + 1057)         // a 1 GiB block (BWT.java:59, the stream header's limit) plus the longest stage header
#define KZ_MAX_BATCH 65535        // blocks per launch: the batched kernels carry the block index in gridDim.y (<= 65535)
int kz_hpin_reserve(kz_ctx* ctx, size_t ints);
static inline size_t kz_align(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Reserve `total` bytes of arena (may reallocate: only call before any sub-allocation).
int kz_arena_reserve(kz_ctx* ctx, size_t total);
void* kz_arena_alloc(kz_ctx* ctx, size_t bytes);   // 256-byte aligned; nullptr on overflow

// A batch of independent blocks resident in HBM: block b lives at base + b*stride.
struct kz_batch {
  int B = 0;            // blocks in the batch
  int maxN = 0;         // largest original block length
  int64_t stride = 0;   // bytes between blocks in each ping-pong buffer
  uint8_t* buf[2] = {nullptr, nullptr};
  int cur = 0;          // which buffer holds the current data
  int32_t* d_len = nullptr;     // [B] current length per block (device)
  int32_t* d_len2 = nullptr;    // [B] next length (stages write here, then swap)
  int32_t* d_flag = nullptr;    // [B] per-stage applied flag (device)
  int32_t* d_dtype = nullptr;   // [B] Global.DataType of each block: the reference's per-block context entry "dataType"
  const int32_t* d_rltEnd = nullptr;   // [B] RLT forward: dst.length of the array the reference's RLT would write this block into (RLT.java:115);
  int rltEndAll = 0;                   //     null: rltEndAll for every block
  std::vector<int32_t> h_len;   // host mirror of d_len
  int slotRot = 0;              // rotation of the SIMD assignment in kz_place_blocks (views launched side by side start on different SIMDs)
  int prio = 0;                 // issue priority of the serial-per-block kernels launched for this view (overlapped decoder schedule)
  std::vector<int32_t> h_cost;  // optional per-block cost hint for serial-per-block stages (length at the previous stage's input)
};

struct KzPlacement { int wpg = 1; int R = 1; std::vector<int> G, off; const int32_t* d_order = nullptr; };
int kz_place_blocks(kz_ctx*, const kz_batch&, KzPlacement&);     // kz_sbrt.hip: cost-aware placement of one-wave-per-block kernels

// ---- stages (each works on the whole batch; returns 0 or -KZ_ERR_*) ----
// forward: reads batch.buf[cur] / d_len, writes buf[cur^1] / d_len and d_flag[b]=1 applied, 0 declined
int kz_stage_bwt_forward(kz_ctx*, kz_batch&);
int kz_stage_bwt_inverse(kz_ctx*, kz_batch&);
int kz_stage_sbrt_forward(kz_ctx*, kz_batch&, int mode);
int kz_stage_sbrt_inverse(kz_ctx*, kz_batch&, int mode);
int kz_sbrt_ranks(kz_ctx*, const uint8_t* src, uint8_t* dst, int64_t stride, const int32_t* d_len, int B, int maxN, int mode);
int kz_stage_srt_forward(kz_ctx*, kz_batch&);
int kz_stage_srt_inverse(kz_ctx*, kz_batch&);
int kz_stage_lz_forward(kz_ctx*, kz_batch&, int extra);
int kz_stage_mm_forward(kz_ctx*, kz_batch&);                    // FSDCodec (kz_mm.hip); reads and writes batch.d_dtype
int kz_stage_mm_inverse(kz_ctx*, kz_batch&, int dstCap);
size_t kz_mm_scratch(int B, int maxN);
int kz_stage_alias_forward(kz_ctx*, kz_batch&, int onlyDNA);    // AliasCodec = PACK / DNA (kz_alias.hip); reads and writes batch.d_dtype
int kz_stage_alias_inverse(kz_ctx*, kz_batch&, int dstCap);
size_t kz_alias_scratch(int B, int maxN, bool decode);
int kz_block_data_types(kz_ctx*, kz_batch&, int init, bool sniff);
int kz_skip_block_flags(kz_ctx*, kz_batch&, int32_t* d_skip);   // the writer's "skipBlocks" test per block (kz_mm.hip)   // batch.d_dtype = init, or the writer's Magic tag per block
int kz_stage_lz_inverse(kz_ctx*, kz_batch&, int extra, int dstCap);
int kz_stage_fpaq_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
int kz_stage_fpaq_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
int kz_block_hashes(kz_ctx*, const uint8_t* data, int64_t stride, const int32_t* d_len, int B, int kind, unsigned long long* d_hash);
size_t kz_srt_scratch(int B, int maxN);
size_t kz_fpaq_scratch(int B, int maxN);
size_t kz_lz_scratch(int B, int maxN);
int kz_stage_zrlt_forward(kz_ctx*, kz_batch&);
int kz_stage_zrlt_inverse(kz_ctx*, kz_batch&, int dstCap);
int kz_stage_rlt_forward(kz_ctx*, kz_batch&, int entropy);     // RLT (kz_rlt.hip); reads and writes batch.d_dtype, reads batch.d_rltEnd / rltEndAll
int kz_stage_rlt_inverse(kz_ctx*, kz_batch&, int dstCap);
size_t kz_rlt_scratch(int B, int maxN);
int kz_stage_lzp_forward(kz_ctx*, kz_batch&);                  // LZP (kz_lzp.hip): one 2^16-int table per block in the arena
int kz_stage_lzp_inverse(kz_ctx*, kz_batch&, int dstCap);
size_t kz_lzp_scratch(int B, int maxN);
int kz_stage_exe_forward(kz_ctx*, kz_batch&);                  // EXE (kz_exe.hip); reads and writes batch.d_dtype
int kz_stage_exe_inverse(kz_ctx*, kz_batch&, int dstCap);
size_t kz_exe_scratch(int B, int maxN, bool decode);
// entropy: reads buf[cur]; writes per-block bitstring at out + b*outStride starting at byte offset
// d_hdrBytes[b]; d_bits[b] = payload bits produced
int kz_stage_ans0_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
// decode: in = bitstrings (payload starts at bit offset d_bitOff[b]); count d_len[b]; writes buf[cur^1]
int kz_stage_ans0_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
// order-1 ANS (kz_ans1.hip): the same contract, 4 MiB chunks
int kz_stage_ans1_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
int kz_stage_ans1_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
size_t kz_ans1_scratch(int B, int maxN, bool decode);
// order-0 range coder (kz_range.hip): the same contract, 32 KiB chunks.  The encoder also writes d_flag[b]: 0 for a block one of
// whose chunks outgrew its payload buffer (d_bits[b] = 0 then), the caller fails that block
int kz_stage_range_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
int kz_stage_range_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
size_t kz_range_scratch(int B, int maxN, bool decode);
int64_t kz_range_max_stream_bytes(int n);  // a single block's RANGE stream at the encoder's payload buffer bound (12.5 bits per byte and the headers)
// CM, the context-model binary coder (kz_cm.hip): the same contract, one chunk per block, blocks below KZ_CM_MAX_BLOCK (kz_cm_host.h).  The encoder
// also writes d_flag[b]: 0 for a block whose stream does not fit its output row or its payload buffer (d_bits[b] = 0 then), the
// caller fails that block
int kz_stage_cm_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
int kz_stage_cm_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);
size_t kz_cm_scratch(int B, int maxN, bool decode);
int kz_stage_huffman_encode(kz_ctx*, kz_batch&, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits);
int kz_stage_huffman_decode(kz_ctx*, kz_batch&, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd);

size_t kz_bwt_forward_scratch(int B, int maxN);
size_t kz_bwt_inverse_scratch(int B, int maxN);
size_t kz_sbrt_scratch(int B, int maxN);
size_t kz_zrlt_scratch(int B, int maxN);
size_t kz_ans_scratch(int B, int maxN);

// per-kernel timing
hipEvent_t kz_ev(kz_ctx* ctx);
void kz_ktimer_flush(kz_ctx* ctx);     // call after the stream has been synchronized
#define KZ_LAUNCH(ctx, kid, kernel, grid, block, ...) do { \
  hipEvent_t a_ = nullptr, b_ = nullptr; \
  if ((ctx)->ktiming) { a_ = kz_ev(ctx); b_ = kz_ev(ctx); (void)hipEventRecord(a_, (ctx)->stream); } \
  hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__); \
  if ((ctx)->ktiming) { (void)hipEventRecord(b_, (ctx)->stream); (ctx)->pending.push_back({a_, b_, kid}); } } while (0)

// ---- host (CPU) stages in front of the GPU chain: TEXT and UTF (kz_text.hip) ----
bool kz_is_host_transform(int type);
bool kz_fast_coder(int entropyType);    // kz_pipe.hip: NONE / ANS0 / HUFFMAN / RANGE, the entropy table's flag
int kz_host_block_data_type(const uint8_t* p, int n, int init);
int kz_host_transform_forward(int type, int entropyType, int blockSize, int* dataType, const uint8_t* src, int n, uint8_t* dst, int dstCap, int* produced);
int kz_host_transform_inverse(int type, int blockSize, const uint8_t* src, int n, uint8_t* dst, int dstCap, int* produced);
// kz_text_gpu.hip: the TEXT inverse of blocks that are still in HBM (done[b] = 1 for the blocks it finished; the others: host stage)
size_t kz_text_gpu_scratch_per_block(int blockSize);
// kz_text_fwd_gpu.hip: the TEXT forward (TextCodec2, or TextCodec1 with variant1) of blocks that sit in HBM (done[b] = 1 for the blocks it finished; the others: host stage)
size_t kz_text_fwd_gpu_scratch(int B, int blockSize, int maxLen, bool variant1);
// kz_utf_fwd_gpu.hip: UTFCodec.forward of the blocks TEXT declined with "dataType" UTF8 (done[b]: 1 applied, 2 declined by the reference's rules, 0 host stage)
int kz_utf_fwd_gpu(kz_ctx* ctx, kz_batch& bt, const std::vector<int32_t>& take, std::vector<int32_t>& done);
bool kz_text_fwd_gpu_applies(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int nBlocks);   // kz_overlap.hip
struct TextFwdJob;
TextFwdJob* kz_text_fwd_gpu_new();
void kz_text_fwd_gpu_free(TextFwdJob*);
int kz_text_fwd_gpu_classify(kz_ctx* ctx, kz_batch& bt, int blockSize, const std::vector<int32_t>& take, std::vector<int32_t>& keeps,
                             std::vector<int32_t>& declined, TextFwdJob& J, bool variant1);
int kz_text_fwd_gpu_launch(kz_ctx* ctx, kz_batch& bt, TextFwdJob& J);
int kz_text_fwd_gpu_finish(kz_ctx* ctx, kz_batch& bt, TextFwdJob& J, std::vector<int32_t>& done);
size_t kz_utf_gpu_scratch_per_block(int maxLen);
int kz_stage_utf_inverse_gpu(kz_ctx* ctx, kz_batch& bt, int dstCap, const std::vector<int32_t>& take, std::vector<int32_t>& done);
int kz_stage_text_inverse_gpu(kz_ctx* ctx, kz_batch& bt, int blockSize, int dstCap, bool variant1, const std::vector<int32_t>& take, std::vector<int32_t>& done, int form);
// run fn(i) for i in [0, n) on host threads (blocks are independent)
void kz_parallel_for(int n, int maxThreads, void (*fn)(int, void*), void* arg);   // kz_host.hip: persistent pool
int kz_usable_cpus();
struct HostPre;
int kz_stage_reserve(kz_ctx* ctx, kz_ctx::Stage& s, size_t need, bool pinned);   // grow-only staging buffer (kz_host.hip)
int32_t kz_encode_blocks_pre(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, const uint8_t* in, int64_t inStride,
                             const int32_t* lengths, int32_t nBlocks, uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind, const HostPre* pre);
// the host stages (TEXT / UTF) of nBlocks blocks in host memory, ahead of kz_encode_blocks_pre (null when the chain has none or they
// cannot be run ahead); kz_host_pre_free releases it
HostPre* kz_host_prestage(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, const uint8_t* hsrc, int64_t hstride,
                          const int32_t* lengths, int32_t nBlocks, int slotId);   // slotId 0/1: the outputs go to the context's pinned hsOut[slotId]
void kz_host_pre_free(HostPre* p);

// ---- the .knz container on device memory (kz_knz_gpu.hip); the callers are in kz_stream_device.hip ----
struct KnzBlk { int64_t pay, bits, src; };   // a block in the container: bit offset of its payload in dst, its W, byte offset of its row
enum { KNZ_WALK_COUNT = 0, KNZ_WALK_END = 1, KNZ_WALK_PREFIX = 2, KNZ_WALK_PAYLOAD = 3 };
int kz_knz_pack(kz_ctx*, const uint8_t* d_rows, const KnzBlk* d_blk, int nb, uint8_t* d_dst, int64_t startBit, int64_t endBit);
int kz_knz_walk(kz_ctx*, const uint8_t* d_src, int64_t n, int64_t startBit, int maxCount, int64_t* d_off, int64_t* d_bits, uint64_t* d_hdr, int64_t* d_res);
int kz_knz_check(kz_ctx*, const uint8_t* d_src, int64_t n, int64_t hdrEnd, const int64_t* d_off, const int64_t* d_bits, int nb, uint64_t* d_hdr, int64_t* d_bad);
int kz_knz_unpack(kz_ctx*, const uint8_t* d_src, int64_t n, const int64_t* d_off, const int64_t* d_bits, int nb, int64_t maxBytes, uint8_t* d_rows, int64_t stride);
// many streams in one call (kz_compress_many_device / kz_decompress_many_device): every table entry carries its own bounds
struct KnzCopy { int64_t src, dst, len; };    // gather / scatter: len bytes from byte offset src of the source base to byte offset dst of the destination base
struct KnzSeg { int64_t dst, endBit, unit0; int32_t blk0, nblk, hdrBytes; uint8_t hdr[28]; };   // pack: a slot (byte offset in dst), its stream's last bit, its first
                                              // 16-byte unit in the launch, its KnzBlk entries (pay relative to the slot) and its stream header
struct KnzSrc { int64_t off, n, startBit, base; int32_t maxCount, cap; };   // walk: the stream src[off .. off + n), first prefix at startBit; entries go to
                                              // base + i for i < cap
struct KnzRow { int64_t seg, n, off, bits, row; };   // unpack: bits from bit off of the stream src[seg .. seg + n) to the row at byte offset `row`
int kz_knz_gather(kz_ctx*, const uint8_t* d_src, const KnzCopy* d_t, int nr, int64_t maxLen, uint8_t* d_rows);
int kz_knz_scatter(kz_ctx*, const uint8_t* d_rows, const KnzCopy* d_t, int nr, int64_t maxLen, uint8_t* d_dst);
int kz_knz_pack_many(kz_ctx*, const uint8_t* d_rows, const KnzSeg* d_seg, int ns, const KnzBlk* d_blk, uint8_t* d_dst, int64_t units);
int kz_knz_heads(kz_ctx*, const uint8_t* d_src, const KnzSrc* d_t, int ns, uint8_t* d_heads);
int kz_knz_walk_many(kz_ctx*, const uint8_t* d_src, const KnzSrc* d_t, int ns, int64_t* d_off, int64_t* d_bits, uint64_t* d_hdr, int64_t* d_res);
int kz_knz_unpack_many(kz_ctx*, const uint8_t* d_src, const KnzRow* d_t, int nr, int64_t maxBytes, uint8_t* d_rows);
// splice (kz_knz_splice_device): a piece is the `bits` bits from bit `off` of the stream src[seg .. seg + n), whose header ends at bit
// hdrEnd; `pay` = the bit offset of its payload in dst (the check does not read it)
struct KnzPiece { int64_t pay, bits, seg, n, off, hdrEnd; };
int kz_knz_check_many(kz_ctx*, const uint8_t* d_src, const KnzPiece* d_pc, int np, int32_t* d_bad);
int kz_knz_splice_launch(kz_ctx*, const uint8_t* d_src, const KnzPiece* d_pc, int np, uint8_t* d_dst, int64_t startBit, int64_t endBit);
// the splice's copy into many destinations in one launch (kz_write_bytes_many_device): span i owns the bits [startBit, endBit) of the
// slot d_dst + dst: the stream header hdr[0 .. hdrBytes) when it is the stream's first (startBit == 0 then), the fields of its pieces
// d_pc[piece0 .. piece0 + npieces) (pay counted from the slot's first bit), zeros up to endBit and to the end of the last byte.  unit0 =
// the span's first 16-byte aligned unit among the launch's (a prefix sum that grows strictly with the span, d_sp[0].unit0 == 0).
struct KnzSpan { int64_t dst, startBit, endBit, unit0; int32_t piece0, npieces, hdrBytes; uint8_t hdr[28]; };
int kz_knz_splice_many(kz_ctx*, const uint8_t* d_src, const KnzSpan* d_sp, int ns, const KnzPiece* d_pc, uint8_t* d_dst, int64_t units);
// the index entries of many streams, each against its own (kz_read_bytes_many_device): entry (off, bits) of the stream src[seg .. seg + n),
// whose header ends at bit hdrEnd; d_hdr[i] = the block-header word as kz_knz_check gives it, d_bad[i] = 0 / 1
struct KnzCheckRow { int64_t seg, n, off, bits, hdrEnd; };
int kz_knz_check_rows(kz_ctx*, const uint8_t* d_src, const KnzCheckRow* d_t, int nr, uint64_t* d_hdr, int64_t* d_bad);
// byte-addressed reads (kz_read_bytes_device): ns segments (kz_knz_host.h) of rows `stride` apart, rowLen bytes of each the block's,
// to their places in d_dst; the launch owns the destination units [unitBase, unitBase + units), d_seg[0].unit0 == unitBase
struct KnzReadSeg;
int kz_knz_read(kz_ctx*, const uint8_t* d_rows, int64_t stride, int rowLen, const KnzReadSeg* d_seg, int ns, uint8_t* d_dst, int64_t unitBase, int64_t units);
// byte-addressed writes (kz_write_bytes_device): ns segments (kz_knz_host.h) of d_data[0 .. dataLen) to their places in rows `stride`
// apart; the launch owns the row units [unitBase, unitBase + units), d_seg[0].unit0 == unitBase
struct KnzWriteSeg;
int kz_knz_write(kz_ctx*, const uint8_t* d_data, int64_t dataLen, const KnzWriteSeg* d_seg, int ns, uint8_t* d_rows, int64_t stride, int64_t unitBase, int64_t units);
// scan (kz_knz_scan_device): the rule (kz_knz_host.h) at every bit position of d_src[0 .. n), in tiles; d_tileOff[0 .. nTiles] = the
// first index of every tile's accepted positions, d_tileOff[nTiles] = their number A; d_cols = kz_knz_scan_cols_bytes(A) bytes for
// the link passes; d_out = four columns (prefix, payload, bits, next) of M = min(A, cap) entries; d_res = (kept entries, head)
struct KnzScanRule;
int64_t kz_knz_scan_tiles_of(const uint8_t* d_src, int64_t n);
size_t kz_knz_scan_cols_bytes(int64_t A);
int kz_knz_scan_count(kz_ctx*, const uint8_t* d_src, int64_t n, const KnzScanRule& R, int64_t nTiles, int32_t* d_cnt, int64_t* d_tileOff);
int kz_knz_scan_links(kz_ctx*, const uint8_t* d_src, int64_t n, const KnzScanRule& R, int64_t nTiles, const int64_t* d_tileOff, uint8_t* d_cols, int64_t A, int mc);
int kz_knz_scan_emit(kz_ctx*, const uint8_t* d_src, int64_t n, const KnzScanRule& R, uint8_t* d_cols, int64_t A, int64_t cap, int64_t* d_out, int64_t M, int64_t* d_res);

// timing helpers
void kz_stage_begin(kz_ctx*, hipEvent_t* e0);
void kz_stage_end(kz_ctx*, hipEvent_t e0, int stageId, int64_t algBytes);
