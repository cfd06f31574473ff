// kz_overlap.hip -- the decoder's overlapped RANK / BWT inverse schedule and the predicates that send a host stage to the device (kz_pipe.h)
#include "kz_pipe.h"

// ---- decoder: RANK / MTFT inverse and BWT inverse of a large batch, overlapped -------------------------------------------
// The RANK inverse is serial per block (one wave per block, no HBM traffic to speak of) and its launch lasts as long as its
// slowest block; the BWT inverse behind it is bandwidth bound.  Run back to back the second waits for blocks the first has long
// finished.  Here the expensive blocks (cost hint = length at the previous stage's input ~ non-zero ranks) take the RANK
// inverse on a side stream while the cheap ones go through RANK inverse AND BWT inverse on the main stream; the expensive
// blocks' BWT inverse follows.  Blocks live in fixed slots of the two ping-pong buffers, so the groups are lengths-masked
// views of the same batch.  Only for batches where both stages apply to the same blocks.
__global__ void k_merge_group(const int32_t* __restrict__ in, const int32_t* __restrict__ len, const int32_t* __restrict__ flag, const int32_t* __restrict__ old,
                              int32_t* __restrict__ lenOut, int32_t* __restrict__ applied, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || !in[b]) return;                                     // other blocks: lenOut (the batch's own lengths) and applied stay
  lenOut[b] = flag[b] > 0 ? len[b] : old[b];
  applied[b] = flag[b] > 0 ? 1 : 0;
}
// the arrays of one group copied into those of a view that holds several groups (their BWT inverses run as one: overlap_finish)
__global__ void k_gather_group(const int32_t* __restrict__ in, const int32_t* __restrict__ len, const int32_t* __restrict__ flag, const int32_t* __restrict__ old,
                               int32_t* __restrict__ mIn, int32_t* __restrict__ mLen, int32_t* __restrict__ mFlag, int32_t* __restrict__ mOld, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || !in[b]) return;
  mIn[b] = 1; mLen[b] = len[b]; mFlag[b] = flag[b]; mOld[b] = old[b];
}
// the TEXT inverse on the device (kz_text_gpu.hip) instead of the host stage: opt-in, KZ_TEXT_GPU=1 (read per call).  Its first
// form is one serial walk per block: 1.07 s for 1 536 text blocks of 4 MiB side by side -- and as long for 384 of them -- where 16
// host CPUs need 0.87 s under the GPU's next chunk; it pays only where the host has next to no CPUs for the process.
// TEXT inverse on the device (kz_text_gpu.hip).  KZ_TEXT_GPU: unset = the row form (three waves per block) for streams whose entropy
// coder selects TextCodec2 (NONE / ANS0 / HUFFMAN / RANGE, TransformFactory.java:275-286) in batches of KZ_TEXT_GPU_MIN blocks or more
// (512: a block takes the kernel ~0.1 s however few there are, the host stage ~10 ms per block and thread), else the host stage;
// 0 = host stage only; 1 = row form, three waves; 2 = serial token walk (both codecs); 3 = row form, one wave (1-3: any batch).
int text_gpu_form(const kz_ctx* ctx, uint32_t entropyType, int nBlocks) {
  if (ctx->sw.textGpu >= 0) return ctx->sw.textGpu;
  return (!kz_fast_coder((int)entropyType) || nBlocks < ctx->sw.textGpuMin) ? 0 : 1;
}
// TEXT forward on the device (kz_text_fwd_gpu.hip): TextCodec2 streams under NONE / ANS0 / HUFFMAN (not RANGE) in batches of KZ_TEXT_FWD_GPU_MIN
// blocks (256) or more -- a block's dictionary walk takes the kernel ~0.1 s however few there are, so small batches stay on the host's
// chunk pipeline (measured with 16 host CPUs, level-exact -l 5 encode of 64 / 128 / 256 / 512 blocks: host 102 / 159 / 293 / 529 ms,
// device 157 / 188 / 247 / 379 ms).  KZ_TEXT_FWD_GPU=0: host stage, =1: any batch size.  (Read per call: the tests force both.)
// TextCodec1 streams (FPAQ / CM / ANS1: the same kernels at TextCodec1's seams) have switches of their own: KZ_TEXT1_FWD_GPU=0: host
// stage, =1: any batch size, unset: batches of KZ_TEXT1_FWD_GPU_MIN blocks (64) or more, 0 = never.  64 is the smallest size measured
// (tools/text1_probe.py, 16 host CPUs, text-heavy mix at 4 MiB blocks in HBM, 64 / 128 / 256 / 512 blocks, median of 5, spread under
// 1 %): level-6 encode host 1966 / 2005 / 2094 / 1696 ms, device 735 / 763 / 816 / 932 ms; TEXT+UTF & FPAQ host 5126 / 5163 / 5195 /
// 3643 ms, device 1786 / 1793 / 1799 / 1821 ms.  The walk itself is ~75 - 85 ms; most of the gain is that a batch on the device path
// is coded in ONE pass, where the host chunk pipeline codes it in thirds (halves from 512 blocks on) and k_fpaq_enc takes ~630 ms
// (level 6) per pass however few blocks it has.
static bool text_fwd_gpu_on(const kz_ctx* ctx, uint32_t entropyType, int nBlocks) {
  if (entropyType == KZ_E_RANGE) return false;                                        // RANGE chains: never measured there
  if (!kz_fast_coder((int)entropyType)) {
    if (ctx->sw.text1FwdGpu >= 0) return ctx->sw.text1FwdGpu == 1;
    return ctx->sw.text1FwdGpuMin > 0 && nBlocks >= ctx->sw.text1FwdGpuMin;
  }
  if (ctx->sw.textFwdGpu >= 0) return ctx->sw.textFwdGpu == 1;
  return nBlocks >= ctx->sw.textFwdGpuMin;
}

static int fuse_min_blocks(const kz_ctx* ctx) { return ctx->sw.fuseMinBlocks; }   // batches below this take the stages one after the other
#define KZ_OVERLAP_MAXG 5
// host side: classes by cost relative to the largest: >= 3/4 | >= 3/8 | >= 3/16 | >= 3/32 | the rest; classes of fewer than 8
// blocks join the class below (the cheapest one: the class above).  false when there is nothing to overlap.
bool overlap_classify(const kz_ctx* ctx, int B, const std::vector<int32_t>& h_mask, const std::vector<int32_t>& cost, Overlap& O) {
  if (B < fuse_min_blocks(ctx)) return false;
  int64_t maxCost = 0;
  for (int b = 0; b < B; b++) if (h_mask[b]) maxCost = std::max<int64_t>(maxCost, cost[b]);
  int nClasses = ctx->sw.overlapClasses;                           // 3: main + two side streams fit HIP's default of 4 hardware queues
  nClasses = std::min(std::max(nClasses, 2), KZ_OVERLAP_MAXG);
  std::vector<int> cls(B, -1);
  int cnt[KZ_OVERLAP_MAXG] = {0};
  for (int b = 0; b < B; b++) {
    if (!h_mask[b]) continue;
    int c = nClasses - 1;                                          // most expensive
    int64_t lim = maxCost * 3;                                     // cost * 4 >= maxCost * 3, then halving
    while (c > 0 && (int64_t)cost[b] * 4 < lim) { c--; lim >>= 1; }
    cls[b] = c;
    cnt[c]++;
  }
  int to[KZ_OVERLAP_MAXG];
  for (int c = 0; c < KZ_OVERLAP_MAXG; c++) to[c] = c;
  for (int c = nClasses - 1; c >= 1; c--)
    if (cnt[c] > 0 && cnt[c] < 8) { cnt[c - 1] += cnt[c]; cnt[c] = 0; for (int k = 0; k < KZ_OVERLAP_MAXG; k++) if (to[k] == c) to[k] = c - 1; }
  if (cnt[0] > 0 && cnt[0] < 8) {                                  // the cheapest class is too small: the next one takes the main stream
    int up = -1;
    for (int c = 1; c < nClasses; c++) if (cnt[c] > 0) { up = c; break; }
    if (up > 0) { cnt[up] += cnt[0]; cnt[0] = 0; for (int k = 0; k < KZ_OVERLAP_MAXG; k++) if (to[k] == 0) to[k] = up; }
  }
  if (ctx->sw.traceSched) {
    int raw[KZ_OVERLAP_MAXG] = {0};
    for (int b = 0; b < B; b++) if (cls[b] >= 0) raw[cls[b]]++;
    fprintf(stderr, "[sched] classes (cheap..expensive) raw %d %d %d %d %d merged %d %d %d %d %d maxCost %lld\n", raw[0], raw[1], raw[2], raw[3], raw[4],
            cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], (long long)maxCost);
  }
  int order[KZ_OVERLAP_MAXG], n = 0;
  for (int c = 0; c < nClasses; c++) if (cnt[c] > 0) order[n++] = c;
  if (n < 2) return false;
  O.groups.resize(n);
  // issue priority of the classes' RANK-inverse waves (s_setprio 3 / 1 / 0).  Round 6: the class whose BWT inverse comes FIRST
  // gets the highest one -- the main stream has nothing to do until that class's last RANK chain has ended, and the long chains of the
  // other classes end under its BWT inverse anyway (bulk decode 595 -> 539 ms; with the 32-bit forms of round 5 the opposite order
  // was the faster one: the incompressible class's chain was then the critical path)
  for (int g = 0; g < n; g++) {
    O.groups[g].in.assign(B, 0);
    O.groups[g].prio = (g == n - 1) ? 2 : (g > 0 ? 1 : 0);          // (the wide schedule: overlap_plan re-assigns by the order of the BWT inverses)
  }
  for (int b = 0; b < B; b++) {
    if (cls[b] < 0) continue;
    const int c = to[cls[b]];
    for (int g = 0; g < n; g++) if (order[g] == c) O.groups[g].in[b] = 1;
  }
  return true;
}
static int overlap_streams(kz_ctx* ctx);
int overlap_alloc(kz_ctx* ctx, int B, Overlap& O) {
  { const int qrc = overlap_streams(ctx); if (qrc) return qrc; }
  for (auto& G : O.groups) {
    int32_t* d = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4 * 5);
    if (!d) { snprintf(ctx->err, sizeof(ctx->err), "overlapped inverse: arena overflow"); return -KZ_ERR_DEVICE; }
    G.d_in = d; G.len = d + B; G.len2 = d + 2 * B; G.flag = d + 3 * B; G.old = d + 4 * B;
    KZ_HIP(hipMemcpyAsync(G.d_in, G.in.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));                        // pageable sources
  return 0;
}
static int overlap_view(kz_ctx* ctx, const kz_batch& bt, OverlapGroup& G) {
  const int B = bt.B;
  G.v = bt;
  G.v.d_len = G.len; G.v.d_len2 = G.len2; G.v.d_flag = G.flag;
  G.v.prio = G.prio;
  for (int b = 0; b < B; b++) if (!G.in[b]) G.v.h_len[b] = 0;
  // the view's device lengths come from the HOST mirror: a block that failed in an earlier stage has length 0 there while the
  // batch's device array still holds its old length, and the stages size their scratch by the host's count of non-empty blocks
  KZ_HIP(hipMemcpyAsync(G.len, G.v.h_len.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  KZ_HIP(hipMemcpyAsync(G.old, G.len, (size_t)B * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}
// Does this process get as many concurrent hardware queues as the wide schedule needs (main + three side streams)?  HIP
// multiplexes its streams over GPU_MAX_HW_QUEUES hardware queues (4 unless the variable says otherwise when the runtime
// starts: the APPLICATION exports GPU_MAX_HW_QUEUES=8 before its first HIP call, the library never touches the environment;
// a caller that forgets it gets the three-stream form below, which this measurement selects), and two streams on one queue run
// one after the other.  Measured once per context: four 2 ms spin kernels on the four streams take 2 ms or 4+.
__global__ void k_spin(long long ticks) {
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
static int overlap_streams(kz_ctx* ctx) {
  for (int i = 0; i < 5; i++) if (!ctx->side[i]) {
    KZ_HIP(hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking));
    KZ_HIP(hipEventCreateWithFlags(&ctx->evJoin[i], hipEventDisableTiming));
  }
  if (ctx->sw.wideQueues >= 0) { ctx->wideNow = ctx->sw.wideQueues; return 0; }   // (the tests force both schedules)
  if (ctx->wideQueues < 0) {
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    hipStream_t q[4] = {ctx->stream, ctx->side[0], ctx->side[1], ctx->side[2]};
    for (int r = 0; r < 2; r++) {                                   // first round: warm-up (queue creation, code load)
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < 4; i++) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, q[i], (long long)200000);   // 100 MHz: 2 ms
      for (int i = 0; i < 4; i++) KZ_HIP(hipStreamSynchronize(q[i]));
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      ctx->wideQueues = ms < 3.5 ? 1 : 0;
    }
    if (ctx->sw.traceSched) fprintf(stderr, "[sched] four streams run %s\n", ctx->wideQueues ? "side by side" : "on shared hardware queues: three-stream schedule");
  }
  ctx->wideNow = ctx->wideQueues;
  return 0;
}
// Order of the groups.  Wide schedule (four concurrent hardware queues): every group's RANK inverse runs on its own side stream;
// the main stream prepares the groups one after the other (entropy decoding + ZRLT inverse, when the caller has not done them
// yet) and then runs the BWT inverses as the RANK inverses finish (HBM-bound kernels with huge grids do not share the GPU with
// another queue's kernels anyway: chains "RANK, BWT" per stream were measured, the BWT stages ran one after the other and
// started late).  The order of the preparation decides which serial chain is on the critical path; it is picked by trying all
// permutations against a three-constant model: RANK inverse = 115 ns per byte of the group's longest ZRLT-coded block, at most 64 ns
// per byte of the block (a serial chain per block; batches this large keep two waves per SIMD), BWT inverse = 40 ps per byte, preparation = 12 ps per
// entropy-coded byte (MI355X, profiles/).  Narrow schedule: two side streams, the cheapest group's RANK inverse on the main
// stream behind all the preparations.
void overlap_plan(kz_ctx* ctx, Overlap& O, const std::vector<int32_t>& zlen, const std::vector<int32_t>& rawp, int blockSize, bool withPre) {
  const int n = (int)O.groups.size();
  O.mainGroup = -1;
  if (!ctx->wideNow || n > 3) {
    O.launchOrder.clear(); O.bwtOrder.clear();
    for (int g = n - 1; g >= 0; g--) O.launchOrder.push_back(g);
    for (int g = 0; g < n; g++) O.bwtOrder.push_back(g);
    O.mainGroup = 0;
    // The main stream runs the cheapest class's RANK inverse itself, behind the last preparation, and the BWT inverses behind that:
    // its chain is what everything else waits for.  With the classes' own priorities (most expensive = highest) that chain ran
    // under the two long ones at their pace and no BWT inverse could begin before all chains had ended (bulk batch, 2048 x 4 MiB,
    // profiles/rankprio_parent_decode_timeline.txt: chains 270 / 282 / 275 ms, all over at 395 ms, then 283 ms of BWT inverses
    // alone, 680 ms).  As in the wide schedule the class whose BWT inverse comes first now issues first and the long chains end
    // under the BWT inverses (profiles/rankprio_new_decode_timeline.txt: cheap class 110 ms, over at 234 ms; skewed bytes 211,
    // incompressible 464 ms, over at 468 ms = 6 ms before the last BWT inverse could start; 533 ms).
    if ((int)zlen.size() > 4 * ctx->numCUs)
      for (size_t i = 0; i < O.bwtOrder.size(); i++) O.groups[O.bwtOrder[i]].prio = i == 0 ? 2 : (i == 1 ? 1 : 0);
    return;
  }
  for (auto& G : O.groups) {
    int64_t maxZ = 0, pre = 0, cnt = 0, raws = 0;
    for (size_t b = 0; b < G.in.size(); b++) if (G.in[b]) { maxZ = std::max<int64_t>(maxZ, zlen[b]); cnt++; raws += rawp[b] ? 1 : 0; pre += rawp[b] ? zlen[b] / 16 : zlen[b]; }
    // round 6: a block whose ranks are nearly all non-zero and mostly >= 64 (ZRLT-coded length ~ its own: incompressible data)
    // runs in the interleaved keyed rows of kz_sbrt_f64.h (blocks up to 8 MiB), rows without ranks >= 64 in the by-position keyed
    // rows.  Measured in the bulk batch (two waves per SIMD, the other classes' waves and the BWT inverses beside them); the class
    // of cheap blocks (three fifths of the batch) takes 1.65 x what its longest block suggests: the factor 1 + blocks / (2 x SIMDs'
    // worth) below.  (Tried and measured slower: the large class cut in two at its median cost on six streams, 643 - 805 ms against
    // 593; the longest chain first, 695 against 665.)
    const bool keyedForms = ctx->sw.sbrtForm != 0 && blockSize <= (1 << 23);
    const bool keyed = keyedForms && maxZ >= (int64_t)blockSize - (blockSize >> 5) && raws * 2 > cnt;   // incompressible (stored raw): ranks of every depth
    const double crowd = 1.0 + 0.55 * (double)cnt / (4.0 * (double)std::max(1, ctx->numCUs));
    // (with the keyed rows: incompressible class 464 ms = 95 ns per byte of the block, skewed bytes 331 ms = at most 65 ns per byte,
    // cheap blocks 232 ms = 86 ns per ZRLT-coded byte, each times the crowding factor)
    if (!keyedForms) G.tRank = 115e-9 * (double)maxZ * crowd;
    else G.tRank = (keyed ? 95e-9 * (double)blockSize : std::min(86e-9 * (double)maxZ, 65e-9 * (double)blockSize)) * crowd;
    G.tBwt = 40e-12 * (double)cnt * (double)blockSize;
    G.tPre = withPre ? 12e-12 * (double)pre : 0.0;
  }
  std::vector<int> perm(n), best;
  for (int i = 0; i < n; i++) perm[i] = i;
  double bestT = 1e30;
  do {
    double t = 0, endR[KZ_OVERLAP_MAXG];
    for (int i = 0; i < n; i++) { t += O.groups[perm[i]].tPre; endR[perm[i]] = t + O.groups[perm[i]].tRank; }
    std::vector<int> byEnd(perm);
    std::sort(byEnd.begin(), byEnd.end(), [&](int a, int b) { return endR[a] < endR[b]; });
    double tb = t;                                                  // the main stream is busy with the preparations until t
    for (int g : byEnd) tb = std::max(tb, endR[g]) + O.groups[g].tBwt;
    if (tb < bestT - 1e-9) { bestT = tb; best = perm; O.bwtOrder = byEnd; }
  } while (std::next_permutation(perm.begin(), perm.end()));
  O.launchOrder = best;
  {
    // Round 6: groups whose RANK chains are (by the model) over before the main stream gets to them have their BWT inverses run as
    // ONE call: the walk of 416 blocks takes 45 ms, of 832 about 80, and the per-call tails and launches are paid once
    // (the two trailing classes of the bulk batch: 2 x 60 -> 85 ms).
    double t = 0, endR[KZ_OVERLAP_MAXG];
    for (int i = 0; i < n; i++) { t += O.groups[O.launchOrder[i]].tPre; endR[O.launchOrder[i]] = t + O.groups[O.launchOrder[i]].tRank; }
    double tb = t;
    O.bwtCalls.clear();
    for (size_t i = 0; i < O.bwtOrder.size();) {
      std::vector<int> call(1, O.bwtOrder[i]);
      const double begin = std::max(tb, endR[O.bwtOrder[i]]);
      double dur = O.groups[O.bwtOrder[i]].tBwt;
      size_t k = i + 1;
      // (only chains over by then: taking in a chain that ends later -- tried with `<= begin + dur` -- holds the call back behind the longest
      // one: bulk decode 544 -> 587 ms)
      while (i > 0 && k < O.bwtOrder.size() && endR[O.bwtOrder[k]] <= begin) { call.push_back(O.bwtOrder[k]); dur += O.groups[O.bwtOrder[k]].tBwt; k++; }
      O.bwtCalls.push_back(call);
      tb = begin + dur;
      i = k;
    }
  }
  if ((int)zlen.size() > 4 * ctx->numCUs)                           // (batches of one wave per SIMD or less: the longest chain keeps the highest priority)
    for (size_t i = 0; i < O.bwtOrder.size(); i++) O.groups[O.bwtOrder[i]].prio = i == 0 ? 2 : (i == 1 ? 1 : 0);
  if (ctx->sw.traceSched) {
    fprintf(stderr, "[sched] plan %.0f ms: launch", bestT * 1e3);
    for (int g : O.launchOrder) fprintf(stderr, " %d(pre %.0f rank %.0f bwt %.0f)", g, O.groups[g].tPre * 1e3, O.groups[g].tRank * 1e3, O.groups[g].tBwt * 1e3);
    fprintf(stderr, " | bwt order"); for (int g : O.bwtOrder) fprintf(stderr, " %d", g); fprintf(stderr, "\n");
  }
}
// RANK inverse of group g: on the main stream for the narrow schedule's main group, else on side stream k (everything queued
// on the main stream so far is waited for)
int overlap_start_rank(kz_ctx* ctx, const kz_batch& bt, int mode, Overlap& O, int g, int k) {
  OverlapGroup& G = O.groups[g];
  int rc = overlap_view(ctx, bt, G);
  if (rc) return rc;
  {                                                                 // the launches so far occupy the first SIMDs of every CU
    int64_t act = 0;
    for (int b = 0; b < bt.B; b++) act += G.in[b] ? 1 : 0;
    G.v.slotRot = (int)((O.started / std::max(1, (bt.B + 7) / 8)) & 3);
    O.started += act;
  }
  if (g == O.mainGroup) { G.ev = -1; return kz_stage_sbrt_inverse(ctx, G.v, mode); }
  G.ev = k;
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  hipStream_t& sd = ctx->side[k];
  std::swap(ctx->stream, sd);
  rc = kz_stage_sbrt_inverse(ctx, G.v, mode);
  if (!rc) { hipError_t e = hipEventRecord(ctx->evJoin[k], ctx->stream); if (e != hipSuccess) rc = -KZ_ERR_DEVICE; }
  std::swap(ctx->stream, sd);
  return rc;
}
// the groups' BWT inverses on the main stream, in the planned order; merges lengths and flags
int overlap_finish(kz_ctx* ctx, Pipe& P, Overlap& O, std::vector<int32_t>& h_applied) {
  kz_batch& bt = P.bt;
  const int B = bt.B;
  hipStream_t st = ctx->stream;
  int rc = 0;
  if (O.bwtCalls.empty()) for (int g : O.bwtOrder) O.bwtCalls.push_back(std::vector<int>(1, g));
  // a call of several groups works on a view of its own: the groups' masks, lengths, flags and old lengths gathered (allocated in
  // front of `mark`: the stages' scratch behind it is given back between the calls)
  struct Merged { OverlapGroup M; bool used = false; };
  std::vector<Merged> merged(O.bwtCalls.size());
  for (size_t c = 0; c < O.bwtCalls.size(); c++) {
    if (O.bwtCalls[c].size() < 2) continue;
    OverlapGroup& M = merged[c].M;
    int32_t* d = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4 * 5);
    if (!d) { snprintf(ctx->err, sizeof(ctx->err), "overlapped inverse: arena overflow"); return -KZ_ERR_DEVICE; }
    M.d_in = d; M.len = d + B; M.len2 = d + 2 * B; M.flag = d + 3 * B; M.old = d + 4 * B;
    merged[c].used = true;
  }
  const size_t mark = ctx->arenaTop;
  for (size_t c = 0; c < O.bwtCalls.size(); c++) {
    const std::vector<int>& call = O.bwtCalls[c];
    for (int g : call) if (O.groups[g].ev >= 0) KZ_HIP(hipStreamWaitEvent(st, ctx->evJoin[O.groups[g].ev], 0));
    ctx->arenaTop = mark;                                           // same stream, in order: the scratch is free again
    if (!merged[c].used) { rc = kz_stage_bwt_inverse(ctx, O.groups[call[0]].v); if (rc) return rc; continue; }
    OverlapGroup& M = merged[c].M;
    M.v = O.groups[call[0]].v;                                      // (same buffers, same `cur`: every view has run one stage)
    KZ_HIP(hipMemsetAsync(M.d_in, 0, (size_t)B * 4 * 5, st));
    for (size_t q = 0; q < call.size(); q++) {
      OverlapGroup& G = O.groups[call[q]];
      if (G.v.cur != M.v.cur) { snprintf(ctx->err, sizeof(ctx->err), "overlapped inverse: views out of step"); return -KZ_ERR_DEVICE; }
      if (q > 0) for (int b = 0; b < B; b++) if (G.in[b]) M.v.h_len[b] = G.v.h_len[b];
      hipLaunchKernelGGL(k_gather_group, dim3((B + 255) / 256), dim3(256), 0, st, G.d_in, G.v.d_len, G.v.d_flag, G.old, M.d_in, M.len, M.flag, M.old, B);
    }
    M.v.d_len = M.len; M.v.d_len2 = M.len2; M.v.d_flag = M.flag;
    rc = kz_stage_bwt_inverse(ctx, M.v);
    if (rc) return rc;
  }
  // every view is back in the buffer it started from (two stages each); the batch's own state is untouched except lengths
  KZ_HIP(hipMemsetAsync(P.d_applied, 0, (size_t)B * 4, st));
  for (size_t c = 0; c < O.bwtCalls.size(); c++) {
    if (merged[c].used) {
      OverlapGroup& M = merged[c].M;
      KZ_LAUNCH(ctx, KID_MASK_LEN, k_merge_group, dim3((B + 255) / 256), dim3(256), M.d_in, M.v.d_len, M.v.d_flag, M.old, bt.d_len, P.d_applied, B);
    } else {
      OverlapGroup& G = O.groups[O.bwtCalls[c][0]];
      KZ_LAUNCH(ctx, KID_MASK_LEN, k_merge_group, dim3((B + 255) / 256), dim3(256), G.d_in, G.v.d_len, G.v.d_flag, G.old, bt.d_len, P.d_applied, B);
    }
  }
  KZ_HIP(hipMemcpyAsync(ctx->hpin + B, P.d_applied, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  rc = sync_lengths(ctx, bt);
  if (rc) return rc;
  h_applied.resize(B);
  for (int b = 0; b < B; b++) h_applied[b] = ctx->hpin[B + b];
  return 0;
}
// returns 1 when it ran both stages (h_applied = blocks both were applied to), 0 when the schedule does not apply, <0 on error
int overlapped_rank_bwt_inverse(kz_ctx* ctx, Pipe& P, int mode, const std::vector<int32_t>& h_mask, const std::vector<int32_t>& cost,
                                       std::vector<int32_t>& h_applied) {
  Overlap O;
  if (!overlap_classify(ctx, P.bt.B, h_mask, cost, O)) return 0;
  int rc = overlap_alloc(ctx, P.bt.B, O);
  if (rc) return rc;
  {
    std::vector<int32_t> none(P.bt.B, 0);
    overlap_plan(ctx, O, P.bt.h_len, none, P.bt.maxN, false);
  }
  for (size_t k = 0; k < O.launchOrder.size(); k++) { rc = overlap_start_rank(ctx, P.bt, mode, O, O.launchOrder[k], (int)k); if (rc) return rc; }
  rc = overlap_finish(ctx, P, O, h_applied);
  return rc ? rc : 1;
}

// does a batch of nBlocks blocks of this chain run its TEXT stage on the device (kz_stream.hip: such chunks are not pre-staged on the host)
bool kz_text_fwd_gpu_applies(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int nBlocks) {
  Chain C;
  chain_split(transformType, C);
  return C.hp > 0 && !ctx->skipBlocks && C.types[0] == KZ_T_TEXT && (C.hp == 1 || C.types[1] == KZ_T_UTF) && text_fwd_gpu_on(ctx, entropyType, nBlocks);
}
