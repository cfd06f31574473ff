// kz_api.hip -- C-ABI entry points (include/kanzi_hip.h) of the context: lifecycle, switches, timers, the asynchronous job queue and
// the single-block calls.  The batched drivers are kz_encode.hip / kz_decode.hip over kz_pipe.h.
#include <dirent.h>
#include "kz_pipe.h"
#include <stdlib.h>
#include <thread>
#include <sched.h>

// =================================================================================================
// context / arena
extern "C" int32_t kz_abi_version(void) { return KZ_ABI_VERSION; }

// The decoder's wide schedule keeps four streams busy side by side; HIP's default is four hardware queues for ALL streams of
// the process.  The library does NOT touch the process environment: the application exports GPU_MAX_HW_QUEUES=8 before its
// first HIP call (bench.py, tests/conftest.py and the Python binding do; a JVM is started with it in its environment,
// INTEGRATION.md 3) or gets the measured three-stream fallback (overlap_streams).
extern "C" kz_ctx* kz_ctx_create(int32_t deviceId) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return nullptr;   // fail loudly: no CPU fallback
  if (deviceId < 0 || deviceId >= ndev) return nullptr;
  if (hipSetDevice(deviceId) != hipSuccess) return nullptr;
  kz_ctx* ctx = new kz_ctx();
  ctx->device = deviceId;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, deviceId) == hipSuccess && cus > 0) ctx->numCUs = cus; }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return nullptr; }
  if (hipHostMalloc((void**)&ctx->hpin, 1 << 20, hipHostMallocDefault) != hipSuccess) { hipStreamDestroy(ctx->stream); delete ctx; return nullptr; }
  ctx->hpinInts = (1 << 20) / 4;
  kz_switches_read(ctx->sw);
  {
    const int hw = (int)std::thread::hardware_concurrency();
    ctx->blockingWaits = ctx->sw.blockingWaits >= 0 ? ctx->sw.blockingWaits : ((hw > 0 && kz_usable_cpus() < hw) ? 1 : 0);
  }
  return ctx;
}
// every environment switch of the library, in one place (kz_internal.h: kz_switches)
void kz_switches_read(kz_switches& s) {
  s = kz_switches();
  auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  auto flag = [](const char* name) { return getenv(name) != nullptr ? 1 : 0; };
  auto digit = [](const char* name, int lo, int hi, int unset) { const char* e = getenv(name); return (e && e[0] >= '0' + lo && e[0] <= '0' + hi) ? e[0] - '0' : unset; };
  { const char* e = getenv("KZ_BLOCKING_WAITS"); s.blockingWaits = e ? (atoi(e) ? 1 : 0) : -1; }
  s.textGpu = digit("KZ_TEXT_GPU", 0, 3, -1);
  s.textGpuMin = num("KZ_TEXT_GPU_MIN", 512);
  s.textFwdGpu = digit("KZ_TEXT_FWD_GPU", 0, 1, -1);
  s.textFwdGpuMin = num("KZ_TEXT_FWD_GPU_MIN", 256);
  s.text1FwdGpu = digit("KZ_TEXT1_FWD_GPU", 0, 1, -1);
  s.text1FwdGpuMin = num("KZ_TEXT1_FWD_GPU_MIN", 64);
  s.utfGpu = digit("KZ_UTF_GPU", 0, 0, 1);
  s.utfFwdGpu = digit("KZ_UTF_FWD_GPU", 0, 1, -1);
  s.textGpuTrace = flag("KZ_TEXT_GPU_TRACE");
  s.fuseMinBlocks = num("KZ_FUSE_MIN_BLOCKS", 32);
  s.overlapClasses = num("KZ_OVERLAP_CLASSES", 3);
  { const char* e = getenv("KZ_WIDE_QUEUES"); s.wideQueues = e ? (atoi(e) ? 1 : 0) : -1; }
  s.noSFirst = flag("KZ_NO_SFIRST");
  s.traceSched = flag("KZ_TRACE_SCHED");
  s.tracePipe = flag("KZ_TRACE_PIPE");
  s.hostChunk = num("KZ_HOST_CHUNK", 0);
  { const int v = num("KZ_HOST_CHUNK_DEC", 512); s.hostChunkDec = v < 8 ? 8 : v; }
  { const char* e = getenv("KZ_HOST_INV_STAGED"); s.hostInvStaged = e ? atoi(e) : -1; }
  s.streamChunk = num("KZ_STREAM_CHUNK", 0);
  s.streamSerial = flag("KZ_STREAM_SERIAL");
  s.readScatter = flag("KZ_READ_SCATTER");
  s.writeGather = flag("KZ_WRITE_GATHER");
  s.bwtTrie = num("KZ_BWT_TRIE", -1); s.bwtTrieWin = num("KZ_BWT_TRIEWIN", -1); s.bwtBuckets = num("KZ_BWT_BUCKETS", -1);
  s.bwtDmax = num("KZ_BWT_DMAX", -1); s.bwtRetire = num("KZ_BWT_RETIRE", -1); s.bwtLazyRank = num("KZ_BWT_LAZYRANK", -1);
  s.bwtLivePart = num("KZ_BWT_LIVEPART", -1);
  s.bwtTrace = flag("KZ_BWT_TRACE");
  s.bwtTestTrieOverflow = digit("KZ_BWT_TEST_TRIE_OVERFLOW", 0, 9, -1);
  s.cmTestRowBytes = num("KZ_CM_TEST_ROW_BYTES", 0);
  { const char* f = getenv("KZ_FPAQ_FORCE"); s.fpaqForce = f ? ((f[0] == 'w' || f[0] == 'W' || f[0] == '1') ? 1 : ((f[0] == 'l' || f[0] == 'L' || f[0] == '2') ? 2 : 0)) : 0; }
  s.sbrtForm = num("KZ_SBRT_FORM", -1);
}
extern "C" void kz_ctx_reload_switches(kz_ctx* ctx) {
  if (!ctx) return;
  kz_switches_read(ctx->sw);
  if (ctx->sw.blockingWaits >= 0) ctx->blockingWaits = ctx->sw.blockingWaits;
}
extern "C" void kz_ctx_destroy(kz_ctx* ctx) {
  if (!ctx) return;
  if (ctx->worker.joinable()) {                                     // queued batches finish first
    { std::lock_guard<std::mutex> g(ctx->qmu); ctx->stopWorker = true; }
    ctx->qcv.notify_all();
    ctx->worker.join();
  }
  hipSetDevice(ctx->device);
  if (ctx->arena) hipFree(ctx->arena);
  for (int i = 0; i < 5; i++) { if (ctx->side[i]) hipStreamDestroy(ctx->side[i]); if (ctx->evJoin[i]) hipEventDestroy(ctx->evJoin[i]); }
  if (ctx->hpin) hipHostFree(ctx->hpin);
  for (int i = 0; i < 2; i++) {
    if (ctx->pinIn[i].p) hipHostFree(ctx->pinIn[i].p);
    if (ctx->pinOut[i].p) hipHostFree(ctx->pinOut[i].p);
    if (ctx->hsIn[i].p) hipHostFree(ctx->hsIn[i].p);
    if (ctx->hsOut[i].p) hipHostFree(ctx->hsOut[i].p);
    if (ctx->tfOut[i].p) hipHostFree(ctx->tfOut[i].p);
    if (ctx->hiAux[i].p) hipFree(ctx->hiAux[i].p);
    if (ctx->hiStream[i]) hipStreamDestroy(ctx->hiStream[i]);
    if (ctx->devIn[i].p) hipFree(ctx->devIn[i].p);
    if (ctx->devOut[i].p) hipFree(ctx->devOut[i].p);
  }
  if (ctx->tfIn.p) hipHostFree(ctx->tfIn.p);
  if (ctx->knzPin.p) hipHostFree(ctx->knzPin.p);
  if (ctx->knzAux.p) hipFree(ctx->knzAux.p);
  if (ctx->tfCopy) hipStreamDestroy(ctx->tfCopy);
  if (ctx->evBlock) hipEventDestroy(ctx->evBlock);
  if (ctx->copyUp) hipStreamDestroy(ctx->copyUp);
  if (ctx->copyDown) hipStreamDestroy(ctx->copyDown);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}
extern "C" int32_t kz_ctx_set_checksum(kz_ctx* ctx, int32_t bits) {
  if (!ctx || (bits != 0 && bits != 32 && bits != 64)) return -KZ_ERR_INVALID_PARAM;
  ctx->checksum = bits == 32 ? 1 : (bits == 64 ? 2 : 0);
  return 0;
}
// ctx map key "skipBlocks" (the reference CLI's --skip): blocks that look incompressible are stored as copy blocks
extern "C" int32_t kz_ctx_set_skip_blocks(kz_ctx* ctx, int32_t on) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  ctx->skipBlocks = on ? 1 : 0;
  return 0;
}
// ctx map key "dataType" (Global.DataType): what a transform instance built with this context would find / leave there
extern "C" int32_t kz_ctx_set_data_type(kz_ctx* ctx, int32_t dataType) {
  if (!ctx || dataType < KZ_DT_UNDEFINED || dataType > KZ_DT_UTF8) return -KZ_ERR_INVALID_PARAM;
  ctx->dataType = dataType;
  return 0;
}
// ctx map keys "blockSize" and "entropy" as TEXT reads them (TextCodec.java:561-575,1068-1081; TransformFactory.java:275-286)
extern "C" int32_t kz_ctx_set_block_size(kz_ctx* ctx, int32_t blockSize) {
  if (!ctx || blockSize < 1024 || blockSize > (1 << 30) || (blockSize & 15)) return -KZ_ERR_BLOCK_SIZE;   // CompressedOutputStream.java:165-174
  ctx->blockSize = blockSize;
  ctx->blockSizeSet = true;
  return 0;
}
extern "C" int32_t kz_ctx_set_entropy(kz_ctx* ctx, uint32_t entropyType) {
  // TPAQX (9) is refused: the reference gives TEXT one more hash bit under it (TextCodec.java:561-575 extraPerf), which the host
  // stage does not model, and no entropy coder in scope is TPAQX
  if (!ctx || entropyType >= 9 || entropyType == 3) return -KZ_ERR_INVALID_CODEC;
  ctx->entropy = (int)entropyType;
  return 0;
}
// every kz_ctx_set_* value back to what a fresh context has (a caller that leaves through an error path need not remember which
// entries of its "map" it had set)
extern "C" int32_t kz_ctx_reset(kz_ctx* ctx) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  ctx->checksum = 0; ctx->skipBlocks = 0; ctx->dataType = KZ_DT_UNDEFINED;
  ctx->blockSize = 4 * 1024 * 1024; ctx->blockSizeSet = false; ctx->entropy = KZ_E_NONE;
  return 0;
}
extern "C" int32_t kz_ctx_get_data_type(kz_ctx* ctx) { return ctx ? ctx->dataType : -KZ_ERR_INVALID_PARAM; }
// N ranks on one host (one process per GPU): keep the process's host threads (TEXT / UTF stages, bit assembly, staging copies)
// on the CPUs next to its GPU.  Reads /sys/bus/pci/devices/<bdf>/local_cpulist; returns the number of CPUs pinned to, 0 when
// the topology is not visible (nothing changed), <0 on error.  Threads created afterwards inherit the mask.
extern "C" int32_t kz_pin_to_device_numa(int32_t deviceId) {
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), deviceId) != hipSuccess) return -KZ_ERR_DEVICE;
  for (char* p = bdf; *p; p++) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bdf);
  FILE* f = fopen(path, "r");
  if (!f) return 0;
  char line[4096] = {0};
  const bool got = fgets(line, sizeof(line), f) != nullptr;
  fclose(f);
  if (!got) return 0;
  cpu_set_t set;
  CPU_ZERO(&set);
  int count = 0;
  for (char* p = line; *p;) {                                       // "0-31,64-95"
    char* e = nullptr;
    const long a = strtol(p, &e, 10);
    if (e == p) break;
    long b = a;
    p = e;
    if (*p == '-') { b = strtol(p + 1, &e, 10); p = e; }
    for (long c = a; c <= b && c < CPU_SETSIZE; c++) { CPU_SET((int)c, &set); count++; }
    if (*p == ',') p++;
  }
  if (count == 0) return 0;
  // every thread the process has at this moment (sched_setaffinity(0, ..) alone would pin the caller and the threads it creates
  // later, leaving a context's job worker or an already running host pool where they were: ADVICE r3); threads created afterwards
  // inherit their creator's mask
  int pinned = 0;
  if (DIR* dir = opendir("/proc/self/task")) {
    while (struct dirent* de = readdir(dir)) {
      const long tid = strtol(de->d_name, nullptr, 10);
      if (tid > 0 && sched_setaffinity((pid_t)tid, sizeof(set), &set) == 0) pinned++;
    }
    closedir(dir);
  }
  if (pinned == 0 && sched_setaffinity(0, sizeof(set), &set) != 0) return 0;
  return count;
}
extern "C" const char* kz_last_error(kz_ctx* ctx) { return ctx ? ctx->err : "null context"; }
extern "C" void* kz_ctx_stream(kz_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// pinned read-back buffer: the batched calls read up to 9 int arrays of B entries back per stage (run_stage: 2B,
// kz_decode_blocks: 4B + 5B); grown here, never indexed beyond hpinInts
int kz_hpin_reserve(kz_ctx* ctx, size_t ints) {
  if (ints <= ctx->hpinInts) return 0;
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  if (ctx->hpin) { hipHostFree(ctx->hpin); ctx->hpin = nullptr; ctx->hpinInts = 0; }
  ints = kz_align(ints + (ints >> 2), 1 << 16);
  KZ_HIP(hipHostMalloc((void**)&ctx->hpin, ints * 4, hipHostMallocDefault));
  ctx->hpinInts = ints;
  return 0;
}

int kz_arena_reserve(kz_ctx* ctx, size_t total) {
  ctx->arenaTop = 0;
  if (total <= ctx->arenaCap) return 0;
  if (ctx->arena) { hipStreamSynchronize(ctx->stream); hipFree(ctx->arena); ctx->arena = nullptr; ctx->arenaCap = 0; }
  total = kz_align(total + (total >> 3), 1 << 20);
  KZ_HIP(hipMalloc((void**)&ctx->arena, total));
  ctx->arenaCap = total;
  return 0;
}
void* kz_arena_alloc(kz_ctx* ctx, size_t bytes) {
  size_t top = kz_align(ctx->arenaTop, 256);
  if (top + bytes > ctx->arenaCap) return nullptr;
  ctx->arenaTop = top + bytes;
  return ctx->arena + top;
}

// ---- timing --------------------------------------------------------------------------------------
extern "C" void kz_set_timing(kz_ctx* ctx, int32_t enable) { ctx->timing = enable != 0; }
extern "C" int32_t kz_get_stage_count(kz_ctx*) { return KZ_MAX_STAGES; }
extern "C" float kz_get_stage_ms(kz_ctx* ctx, int32_t s) { return (s >= 0 && s < KZ_MAX_STAGES) ? ctx->stageMs[s] : 0.f; }
extern "C" int64_t kz_get_stage_alg_bytes(kz_ctx* ctx, int32_t s) { return (s >= 0 && s < KZ_MAX_STAGES) ? ctx->stageAlgBytes[s] : 0; }
extern "C" void kz_reset_timing(kz_ctx* ctx) { for (int i = 0; i < KZ_MAX_STAGES; i++) { ctx->stageMs[i] = 0; ctx->stageAlgBytes[i] = 0; } }

hipEvent_t kz_ev(kz_ctx* ctx) {
  if (!ctx->evPool.empty()) { hipEvent_t e = ctx->evPool.back(); ctx->evPool.pop_back(); return e; }
  hipEvent_t e; hipEventCreate(&e); return e;
}
void kz_ktimer_flush(kz_ctx* ctx) {
  for (auto& p : ctx->pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) { ctx->kMs[p.id] += ms; ctx->kLaunches[p.id]++; if (ms > ctx->kMaxMs[p.id]) ctx->kMaxMs[p.id] = ms; }
    ctx->evPool.push_back(p.e0); ctx->evPool.push_back(p.e1);
  }
  ctx->pending.clear();
}
extern "C" void kz_set_kernel_timing(kz_ctx* ctx, int32_t enable) { ctx->ktiming = enable != 0; }
extern "C" int32_t kz_get_kernel_count(void) { return KID_COUNT; }
extern "C" const char* kz_get_kernel_name(int32_t id) { static const char* n[] = KZ_KERNEL_NAMES; return (id >= 0 && id < KID_COUNT) ? n[id] : ""; }
extern "C" double kz_get_kernel_ms(kz_ctx* ctx, int32_t id) { return (id >= 0 && id < KID_COUNT) ? ctx->kMs[id] : 0.0; }
extern "C" double kz_get_kernel_max_ms(kz_ctx* ctx, int32_t id) { return (id >= 0 && id < KID_COUNT) ? ctx->kMaxMs[id] : 0.0; }
extern "C" int64_t kz_get_kernel_launches(kz_ctx* ctx, int32_t id) { return (id >= 0 && id < KID_COUNT) ? ctx->kLaunches[id] : 0; }
extern "C" void kz_reset_kernel_timing(kz_ctx* ctx) { for (int i = 0; i < KID_COUNT; i++) { ctx->kMs[i] = 0; ctx->kMaxMs[i] = 0; ctx->kLaunches[i] = 0; } }

void kz_stage_begin(kz_ctx* ctx, hipEvent_t* e0) {
  *e0 = nullptr;
  if (!ctx->timing) return;
  hipEventCreate(e0);
  hipEventRecord(*e0, ctx->stream);
}
void kz_stage_end(kz_ctx* ctx, hipEvent_t e0, int stageId, int64_t algBytes) {
  if (!ctx->timing || !e0) return;
  hipEvent_t e1; hipEventCreate(&e1);
  hipEventRecord(e1, ctx->stream);
  hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1);
  ctx->stageMs[stageId] += ms; ctx->stageAlgBytes[stageId] += algBytes;
  hipEventDestroy(e0); hipEventDestroy(e1);
}


// =================================================================================================
// asynchronous batches: kz_submit_encode_blocks / kz_submit_decode_blocks queue the same call on the context's worker thread
// and return at once; kz_wait collects the call's return code.  A context runs its jobs one at a time in submission order
// (it owns one stream and one arena); overlap comes from a second context: one host thread can keep the H2D copies and the
// encode of batch k+1 on context A running under the decode of batch k on context B ("two streams"), which is how
// the reference's task pool overlaps blocks (K/io/CompressedOutputStream.java:541-566).
static void ctx_worker(kz_ctx* ctx) {
  for (;;) {
    std::pair<int64_t, std::function<int32_t()>> job;
    {
      std::unique_lock<std::mutex> lk(ctx->qmu);
      ctx->qcv.wait(lk, [&] { return ctx->stopWorker || !ctx->queue.empty(); });
      if (ctx->queue.empty()) return;                               // stop requested and nothing left
      job = std::move(ctx->queue.front());
      ctx->queue.pop_front();
    }
    const int32_t rc = job.second();
    { std::lock_guard<std::mutex> g(ctx->qmu); ctx->finished[job.first] = rc; }
    ctx->qcv.notify_all();
  }
}
static int64_t ctx_submit(kz_ctx* ctx, std::function<int32_t()> fn) {
  std::lock_guard<std::mutex> g(ctx->qmu);
  if (!ctx->worker.joinable()) ctx->worker = std::thread(ctx_worker, ctx);
  const int64_t id = ctx->nextJob++;
  ctx->queue.emplace_back(id, std::move(fn));
  ctx->qcv.notify_all();
  return id;
}
extern "C" int64_t kz_submit_encode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType,
                                           const uint8_t* in, int64_t inStride, const int32_t* lengths, int32_t nBlocks,
                                           uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind) {
  const int32_t bsz = encode_block_size(ctx, transformType);      // the context's "blockSize" entry NOW, not when the job runs
  if (bsz < 0) return bsz;
  return ctx_submit(ctx, [=]() { return kz_encode_blocks_pre(ctx, transformType, entropyType, bsz, in, inStride, lengths, nBlocks, out, outStride, results, memKind, nullptr); });
}
extern "C" int64_t kz_submit_decode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                           const uint8_t* in, int64_t inStride, const int64_t* bitLengths, int32_t nBlocks,
                                           uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  return ctx_submit(ctx, [=]() { return kz_decode_blocks(ctx, transformType, entropyType, blockSize, in, inStride, bitLengths, nBlocks, out, outStride, results, memKind); });
}
extern "C" int32_t kz_wait(kz_ctx* ctx, int64_t job) {
  if (!ctx || job <= 0) return -KZ_ERR_INVALID_PARAM;
  std::unique_lock<std::mutex> lk(ctx->qmu);
  if (job >= ctx->nextJob) return -KZ_ERR_INVALID_PARAM;
  if (job < ctx->collectedBelow || ctx->collected.count(job)) return -KZ_ERR_INVALID_PARAM;   // a job's result is handed out once
  ctx->qcv.wait(lk, [&] { return ctx->finished.count(job) != 0; });
  const int32_t rc = ctx->finished[job];
  ctx->finished.erase(job);
  ctx->collected.insert(job);
  while (ctx->collected.count(ctx->collectedBelow)) { ctx->collected.erase(ctx->collectedBelow); ctx->collectedBelow++; }
  return rc;
}
extern "C" int32_t kz_poll(kz_ctx* ctx, int64_t job) {            // 1 = finished (kz_wait will not block), 0 = queued or running
  if (!ctx || job <= 0) return -KZ_ERR_INVALID_PARAM;
  std::lock_guard<std::mutex> g(ctx->qmu);
  if (job >= ctx->nextJob) return -KZ_ERR_INVALID_PARAM;
  if (job < ctx->collectedBelow || ctx->collected.count(job)) return -KZ_ERR_INVALID_PARAM;
  return ctx->finished.count(job) ? 1 : 0;
}

// =================================================================================================
// single-block mirrors of ByteTransform / EntropyEncoder / EntropyDecoder (host buffers)
static int32_t transform_one(kz_ctx* ctx, uint32_t type, bool forward, const uint8_t* src, int32_t n, uint8_t* dst, int32_t dstCap, int32_t* produced) {
  if (!ctx || !src || !dst || !produced || n < 0) return -KZ_ERR_INVALID_PARAM;
  *produced = 0;
  if (n == 0) return 1;                                             // every reference codec: length 0 -> true
  if (!transform_row((int)type) || type == KZ_T_NONE) { snprintf(ctx->err, sizeof(ctx->err), "transform %u has no HIP stage", type); return -KZ_ERR_INVALID_CODEC; }
  if (forward && dstCap < kz_transform_max_encoded_len(type, n)) return 0;   // e.g. ZRLT.java:68, BWTBlockCodec.java:84-86
  if (host_stage((int)type)) {                                     // TEXT, UTF: host stages, no GPU involved
    int dt = ctx->dataType;
    const int r = forward ? kz_host_transform_forward((int)type, ctx->entropy, ctx->blockSize, &dt, src, n, dst, dstCap, produced)
                          : kz_host_transform_inverse((int)type, ctx->blockSize, src, n, dst, dstCap, produced);
    if (forward) ctx->dataType = dt;
    if (!r) *produced = 0;
    return r ? 1 : 0;
  }
  KZ_HIP(hipSetDevice(ctx->device));
  Pipe P;
  const int maxLen = std::max(kz_transform_max_encoded_len(type, n), std::max(dstCap, n));
  ChainSpec CS; CS.nb = 1; CS.types[0] = (int)type; CS.entropy = KZ_E_NONE;
  int rc = pipe_setup(ctx, P, 1, maxLen, 0, !forward, CS);
  if (rc) return rc;
  kz_batch& bt = P.bt;
  hipStream_t st = ctx->stream;
  KZ_HIP(hipMemcpyAsync(bt.buf[0], src, (size_t)n, hipMemcpyHostToDevice, st));
  bt.h_len[0] = n;
  KZ_HIP(hipMemcpyAsync(bt.d_len, &n, 4, hipMemcpyHostToDevice, st));
  bt.rltEndAll = dstCap;                                            // RLT forward: dst.length (the Java adapter passes the array's length)
  // the instance's context entry "dataType" (kz_ctx_set_data_type): read by MM, LZ/LZX and RLT forward, rewritten by MM and RLT
  rc = kz_block_data_types(ctx, bt, ctx->dataType, false);
  if (rc) return rc;
  std::vector<int32_t> mask(1, 1), applied;
  rc = run_stage(ctx, P, mask, applied, [&](kz_batch& x) { return run_transform_stage(ctx, x, (int)type, forward, dstCap, ctx->entropy); });
  if (rc) return rc;
  if (forward) {
    int32_t dt = 0;
    KZ_HIP(hipMemcpyAsync(&dt, bt.d_dtype, 4, hipMemcpyDeviceToHost, st));
    KZ_HIP(kz_stream_sync(ctx, st));
    ctx->dataType = dt;
  }
  if (applied[0] < 0) { snprintf(ctx->err, sizeof(ctx->err), "transform %u: the reference codec throws on this block (LZ token buffer)", type); return -KZ_ERR_PROCESS_BLOCK; }
  if (!applied[0]) return 0;
  if (bt.h_len[0] > dstCap) return 0;
  *produced = bt.h_len[0];
  if (bt.h_len[0] > 0) KZ_HIP(hipMemcpyAsync(dst, bt.buf[bt.cur], (size_t)bt.h_len[0], hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  return 1;
}
extern "C" int32_t kz_transform_forward(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n, uint8_t* dst, int32_t dstCap, int32_t* produced) {
  return transform_one(ctx, type, true, src, n, dst, dstCap, produced);
}
extern "C" int32_t kz_transform_inverse(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n, uint8_t* dst, int32_t dstCap, int32_t* produced) {
  return transform_one(ctx, type, false, src, n, dst, dstCap, produced);
}

extern "C" int64_t kz_entropy_encode(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n, uint8_t* out, int64_t outCapBytes) {
  if (!ctx || !src || !out || n < 0) return -KZ_ERR_INVALID_PARAM;
  const EntropyRow* E = entropy_row(type); if (!E) return -KZ_ERR_INVALID_CODEC;
  if (E->blockLimit && n >= E->blockLimit) { snprintf(ctx->err, sizeof(ctx->err), "cm encode: block of %d bytes: CM blocks go up to (1 << 26) - 1 bytes", n); return -KZ_ERR_INVALID_CODEC; }
  if (n == 0) {
    // encode() of nothing writes nothing; FPAQ's dispose() still flushes its 56-bit low register, all zero but the
    // 24 padding ones (FPAQEncoder.java:232-238): the call stands for encode + dispose
    if (!E->flushEmpty) return 0;                                        // (BinaryEntropyEncoder.java:250-255 for CM: the same tail)
    if (outCapBytes < 7) return -KZ_ERR_INVALID_PARAM;
    const uint8_t flush[7] = {0, 0, 0, 0, 0xFF, 0xFF, 0xFF};
    memcpy(out, flush, 7);
    return 56;
  }
  KZ_HIP(hipSetDevice(ctx->device));
  Pipe P;
  const int64_t oS = E->streamBytes(n);
  ChainSpec CS; CS.nb = 0; CS.entropy = (int)type;
  int rc = pipe_setup(ctx, P, 1, n, oS + 256, false, CS);
  if (rc) return rc;
  kz_batch& bt = P.bt;
  hipStream_t st = ctx->stream;
  u8* d_out = (u8*)kz_arena_alloc(ctx, (size_t)oS);
  int32_t* d_hdr = (int32_t*)kz_arena_alloc(ctx, 64);
  int64_t* d_bits = (int64_t*)kz_arena_alloc(ctx, 64);
  if (!d_bits) return -KZ_ERR_DEVICE;
  KZ_HIP(hipMemcpyAsync(bt.buf[0], src, (size_t)n, hipMemcpyHostToDevice, st));
  bt.h_len[0] = n;
  KZ_HIP(hipMemcpyAsync(bt.d_len, &n, 4, hipMemcpyHostToDevice, st));
  KZ_HIP(hipMemsetAsync(d_out, 0, (size_t)oS, st));
  KZ_HIP(hipMemsetAsync(d_hdr, 0, 64, st));
  int64_t bits = 0;
  if (E->encode) {
    rc = E->encode(ctx, bt, d_out, oS, d_hdr, d_bits);
    if (rc) return rc;
    if (E->overflow) {
      int32_t ok = 1;
      KZ_HIP(hipMemcpyAsync(&ok, bt.d_flag, 4, hipMemcpyDeviceToHost, st));
      KZ_HIP(kz_stream_sync(ctx, st));
      if (!ok) { snprintf(ctx->err, sizeof(ctx->err), "%s", E->overflow); return -KZ_ERR_PROCESS_BLOCK; }
    }
    KZ_HIP(hipMemcpyAsync(&bits, d_bits, 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(kz_stream_sync(ctx, st));
  } else {
    KZ_HIP(hipMemcpyAsync(d_out, bt.buf[0], (size_t)n, hipMemcpyDeviceToDevice, st));
    bits = 8LL * n;
  }
  const int64_t nbytes = (bits + 7) >> 3;
  if (nbytes > outCapBytes) return -KZ_ERR_WRITE_FILE;
  KZ_HIP(hipMemcpyAsync(out, d_out, (size_t)nbytes, hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  return bits;
}

extern "C" int32_t kz_entropy_decode(kz_ctx* ctx, uint32_t type, const uint8_t* in, int64_t inBits, uint8_t* dst, int32_t count, int64_t* bitsConsumed) {
  if (!ctx || !in || !dst || count < 0) return -KZ_ERR_INVALID_PARAM;
  const EntropyRow* E = entropy_row(type); if (!E) return -KZ_ERR_INVALID_CODEC;
  if (E->blockLimit && count >= E->blockLimit) { snprintf(ctx->err, sizeof(ctx->err), "cm decode: block of %d bytes: CM blocks go up to (1 << 26) - 1 bytes", count); return -KZ_ERR_INVALID_CODEC; }
  if (bitsConsumed) *bitsConsumed = 0;
  if (count == 0) return 0;
  KZ_HIP(hipSetDevice(ctx->device));
  Pipe P;
  const int64_t inBytes = (inBits + 7) >> 3;
  const int64_t inS = (int64_t)kz_align((size_t)inBytes + 64, 256);
  ChainSpec CS; CS.nb = 0; CS.entropy = (int)type;
  int rc = pipe_setup(ctx, P, 1, count, inS + 256, true, CS);
  if (rc) return rc;
  kz_batch& bt = P.bt;
  hipStream_t st = ctx->stream;
  u8* d_in = (u8*)kz_arena_alloc(ctx, (size_t)inS);
  int64_t* d_off = (int64_t*)kz_arena_alloc(ctx, 64);
  if (!d_off) return -KZ_ERR_DEVICE;
  KZ_HIP(hipMemsetAsync(d_in, 0, (size_t)inS, st));
  KZ_HIP(hipMemcpyAsync(d_in, in, (size_t)inBytes, hipMemcpyHostToDevice, st));
  int64_t h[2] = {0, inBits};
  KZ_HIP(hipMemcpyAsync(d_off, h, 16, hipMemcpyHostToDevice, st));
  bt.h_len[0] = count;
  KZ_HIP(hipMemcpyAsync(bt.d_len, &count, 4, hipMemcpyHostToDevice, st));
  if (E->decode) {
    ctx->d_endBits = (long long*)(d_off + 2);
    rc = E->decode(ctx, bt, d_in, inS, d_off, d_off + 1);
    ctx->d_endBits = nullptr;
    if (rc) return rc;
    int32_t flag = 0;
    long long used = 0;
    KZ_HIP(hipMemcpyAsync(&flag, bt.d_flag, 4, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(&used, d_off + 2, 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(kz_stream_sync(ctx, st));
    if (!flag) return -KZ_ERR_PROCESS_BLOCK;
    if (bitsConsumed) *bitsConsumed = (int64_t)used;
    KZ_HIP(hipMemcpyAsync(dst, bt.buf[bt.cur], (size_t)count, hipMemcpyDeviceToHost, st));
  } else {
    if (inBits < 8LL * count) return -KZ_ERR_PROCESS_BLOCK;
    KZ_HIP(hipMemcpyAsync(dst, d_in, (size_t)count, hipMemcpyDeviceToHost, st));
    if (bitsConsumed) *bitsConsumed = 8LL * count;
  }
  KZ_HIP(kz_stream_sync(ctx, st));
  return count;
}
