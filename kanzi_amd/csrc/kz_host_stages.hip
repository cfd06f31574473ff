// kz_host_stages.hip -- the host TEXT / UTF stages of the batched drivers (kz_pipe.h)
#include "kz_pipe.h"

// host (CPU) stages: TEXT and UTF lead the chains of the reference's levels 3, 5 and 6.  They are sequential dictionary coders
// (kz_text.hip); the batched calls run them per block on host threads, in front of the GPU stages when encoding and behind
// them when decoding, and carry their skip flags and the block's "dataType" entry through like Sequence does.
struct HostFwd {
  const int* types; int hp; int entropy; int cap; int blockSize;
  const uint8_t* hsrc; int64_t hstride;             // the blocks in host memory
  const int32_t* lengths; const int32_t* copy;      // copy: blocks the chain does not apply to (null: those of <= 15 bytes)
  HostPre* P;
  const uint8_t* const* ptrs = nullptr;             // a LIST of blocks instead (block k at ptrs[k]; hsrc / hstride unused)
  const int32_t* first = nullptr;                   // list form: the stages in front of first[k] are done with block k (they declined:
  const int32_t* dt0 = nullptr;                     //            data untouched, skip bits set) and left the "dataType" dt0[k]
};
// blocks that went through a TEXT / UTF stage on a HOST thread since the last reset (process-wide; bench.py reports them next to the
// stage's wall time, which includes the device forms' kernels): [0] forward, [1] inverse
static std::atomic<int64_t> g_hostStageBlocks[2];
extern "C" int64_t kz_host_stage_blocks(int32_t inverse, int32_t reset) {
  std::atomic<int64_t>& c = g_hostStageBlocks[inverse ? 1 : 0];
  return reset ? c.exchange(0) : c.load();
}
static void host_forward_block(int b, void* arg) {
  HostFwd& H = *(HostFwd*)arg;
  HostPre& P = *H.P;
  const int n = H.lengths[b];
  P.outLen[b] = n;
  P.dtype[b] = KZ_DT_UNDEFINED;
  P.skip[b] = 0xFF;
  P.changed[b] = 0;
  if (n == 0 || (H.copy ? H.copy[b] != 0 : n <= 15)) return;
  g_hostStageBlocks[0]++;
  static thread_local std::vector<uint8_t> bufA;
  if ((int)bufA.size() < H.cap + 64) bufA.resize((size_t)H.cap + 64);
  const uint8_t* const origin = H.ptrs ? H.ptrs[b] : H.hsrc + (int64_t)b * H.hstride;
  const uint8_t* cur = origin;
  const int i0 = H.first ? H.first[b] : 0;
  int dt = i0 > 0 ? H.dt0[b] : kz_host_block_data_type(cur, n, KZ_DT_UNDEFINED);   // CompressedOutputStream.java:795-804
  int len = n;
  uint8_t* mine = P.store + (int64_t)b * P.slot;
  uint8_t* out = mine;                                                  // ping-pong between the block's slot and a scratch buffer
  for (int i = i0; i < H.hp; i++) {
    int produced = 0;
    if (!kz_host_transform_forward(H.types[i], H.entropy, H.blockSize, &dt, cur, len, out, H.cap, &produced)) continue;   // declined: data untouched
    P.skip[b] &= ~(1 << (7 - i));
    cur = out; len = produced;
    out = (out == mine) ? bufA.data() : mine;
  }
  P.dtype[b] = dt;
  if (cur != origin) {                                                  // a stage applied
    if (cur != mine) memcpy(mine, cur, (size_t)len);
    P.changed[b] = 1;
    P.outLen[b] = len;
  }
}
int64_t host_pre_slot(int cap) { return (int64_t)kz_align((size_t)cap + 64, 64); }
HostPre HostPre::view(int b0, int cnt) const {
  HostPre v;
  v.outLen.assign(outLen.begin() + b0, outLen.begin() + b0 + cnt);
  v.skip.assign(skip.begin() + b0, skip.begin() + b0 + cnt);
  v.dtype.assign(dtype.begin() + b0, dtype.begin() + b0 + cnt);
  v.changed.assign(changed.begin() + b0, changed.begin() + b0 + cnt);
  v.store = store + (int64_t)b0 * slot; v.slot = slot; v.pinned = pinned;
  return v;
}
// P sized for K results; the slots in `store`, or in memory of P's own (uninitialised: only the bytes a stage writes are touched)
static HostFwd host_fwd_make(const Chain& C, int blockSize, int cap, int K, HostPre& P, uint8_t* store) {
  P.outLen.assign(K, 0); P.skip.assign(K, 0xFF); P.dtype.assign(K, 0); P.changed.assign(K, 0);
  P.slot = host_pre_slot(cap);
  if (store) P.store = store;
  else { P.own.reset(new uint8_t[(size_t)P.slot * (size_t)std::max(K, 1) + 64]); P.store = P.own.get(); }
  HostFwd H;
  H.types = C.types; H.hp = C.hp; H.entropy = C.spec.entropy; H.cap = cap; H.blockSize = blockSize; H.P = &P;
  return H;
}
// runs the chain's host stages over B blocks in host memory
void host_prestage(const Chain& C, int blockSize, int cap, const uint8_t* hsrc, int64_t hstride, const int32_t* lengths, const int32_t* copy, int B,
                   HostPre& P, uint8_t* store) {
  HostFwd H = host_fwd_make(C, blockSize, cap, B, P, store);
  P.pinned = store != nullptr;
  H.hsrc = hsrc; H.hstride = hstride; H.lengths = lengths; H.copy = copy;
  kz_parallel_for(B, KZ_HOST_STAGE_THREADS, host_forward_block, &H);
}
void host_prestage_list(const Chain& C, int blockSize, int cap, const std::vector<const uint8_t*>& ptrs, const std::vector<int32_t>& lengths, HostPre& P,
                        uint8_t* store, const std::vector<int32_t>* first, const std::vector<int32_t>* dt0) {
  const int K = (int)ptrs.size();
  HostFwd H = host_fwd_make(C, blockSize, cap, K, P, store);   // (P.pinned stays false: that flag selects the gather kernel, which indexes slots by block)
  if (K == 0) return;
  std::vector<int32_t> none(K, 0);
  H.hsrc = nullptr; H.hstride = 0; H.lengths = lengths.data(); H.copy = none.data(); H.ptrs = ptrs.data();
  if (first && dt0) { H.first = first->data(); H.dt0 = dt0->data(); }
  kz_parallel_for(K, KZ_HOST_STAGE_THREADS, host_forward_block, &H);
}
// (called off the context's thread by kz_stream.hip: the split alone, no error text; a chain the encoder refuses is refused there)
HostPre* kz_host_prestage(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, const uint8_t* hsrc, int64_t hstride,
                          const int32_t* lengths, int32_t nBlocks, int slotId) {
  Chain C;
  chain_split(transformType, C);
  C.spec.entropy = (int)entropyType;
  if (C.hp == 0 || ctx->skipBlocks || nBlocks <= 0) return nullptr;   // ("skipBlocks": the copy decision comes from the device first)
  int maxN = 0;
  for (int b = 0; b < nBlocks; b++) maxN = std::max(maxN, lengths[b]);
  HostPre* P = new HostPre();
  const int cap = seq_max_len(C.types, C.nb, maxN);
  uint8_t* store = nullptr;
  if (slotId >= 0 && slotId < 2 && hipSetDevice(ctx->device) == hipSuccess &&
      kz_stage_reserve(ctx, ctx->hsOut[slotId], (size_t)host_pre_slot(cap) * (size_t)nBlocks + 64, true) == 0) store = ctx->hsOut[slotId].p;
  host_prestage(C, blockSize, cap, hsrc, hstride, lengths, nullptr, nBlocks, *P, store);
  return P;
}
void kz_host_pre_free(HostPre* p) { delete p; }
void host_inv_make(HostInv& H, const kz_ctx* ctx, const Chain& C, int blockSize, int cap, uint8_t* slots, int64_t stride, bool hostMem, int32_t* len,
                   const int32_t* skip, int32_t* status) {
  H.device = ctx->device; H.types = C.types; H.hp = C.hp; H.blockSize = blockSize; H.cap = cap;
  H.dbuf = slots; H.dstride = stride; H.slotCap = stride; H.hostMem = hostMem;
  H.len = len; H.skip = skip; H.status = status;
}
void host_inverse_block(int b, void* arg) {
  HostInv& H = *(HostInv*)arg;
  int len = H.len[b];
  if (H.status[b] || len <= 0) return;
  bool any = false;
  for (int i = 0; i < H.hp; i++) any |= !(H.skip[b] & (1 << (7 - i)));
  if (!any) return;
  g_hostStageBlocks[1]++;
  static thread_local std::vector<uint8_t> bufA, bufB;
  const size_t need = (size_t)std::max(H.cap, len) + 64;
  if (bufA.size() < need) { bufA.resize(need); bufB.resize(need); }
  uint8_t* slot = H.pin ? H.pin + (int64_t)b * H.pinSlot : H.dbuf + (int64_t)b * H.dstride;
  const bool hostSlot = H.hostMem || H.pin != nullptr;
  uint8_t* cur = bufA.data();
  uint8_t* out = bufB.data();
  if (H.pin) { cur = slot; out = bufA.data(); }                         // read the pinned slot in place, first output to a private buffer
  else if (H.hostMem) memcpy(bufA.data(), slot, (size_t)len);
  else if (hipSetDevice(H.device) != hipSuccess || hipMemcpy(bufA.data(), slot, (size_t)len, hipMemcpyDeviceToHost) != hipSuccess) { H.fail = 1; return; }
  for (int i = H.hp - 1; i >= 0; i--) {                                 // Sequence.inverse: last applied first
    if (H.skip[b] & (1 << (7 - i))) continue;
    int produced = 0;
    if (!kz_host_transform_inverse(H.types[i], H.blockSize, cur, len, out, H.cap, &produced)) { H.status[b] = -KZ_ERR_PROCESS_BLOCK; H.len[b] = 0; return; }
    len = produced;
    if (cur == slot) { cur = out; out = bufB.data(); }                  // (staged form) the slot itself is never an output buffer
    else std::swap(cur, out);
  }
  if ((int64_t)len > H.slotCap) { H.status[b] = -KZ_ERR_PROCESS_BLOCK; H.len[b] = 0; return; }   // more than a block: "incorrectly decompressed"
  if (hostSlot) { if (cur != slot) memcpy(slot, cur, (size_t)len); }
  else if (hipMemcpy(slot, cur, (size_t)len, hipMemcpyHostToDevice) != hipSuccess) { H.fail = 1; return; }
  H.len[b] = len;
}
// The host inverse stages of one chunk whose blocks live in HBM: ONE gather kernel brings the blocks a host stage applies to into
// pinned slots (exact lengths), the host pool decodes them there, ONE scatter kernel puts the results back.  Runs on its own stream
// beside the main stream's next chunk.  (Before: a synchronous D2H and H2D copy per block.)
struct HostInvSub { HostInv* H; int b0; };
static void host_inverse_block_sub(int i, void* arg) { HostInvSub& S = *(HostInvSub*)arg; host_inverse_block(S.b0 + i, S.H); }
void host_inverse_chunk_staged(kz_ctx* ctx, HostInv* H, int cnt, int ring) {
  // d_aux: [0, cnt) lengths in, [cnt, 2 cnt) mask in, [2 cnt, 3 cnt) lengths out, [3 cnt, 4 cnt) mask out
  std::vector<int32_t> hm((size_t)cnt * 4);
  int any = 0;
  for (int b = 0; b < cnt; b++) {
    bool need = !H->status[b] && H->len[b] > 0;
    if (need) { bool a = false; for (int i = 0; i < H->hp; i++) a |= !(H->skip[b] & (1 << (7 - i))); need = a; }
    hm[b] = H->len[b]; hm[cnt + b] = need ? 1 : 0; any |= need ? 1 : 0;
  }
  if (!any) return;
  hipStream_t hs = ctx->hiStream[ring];
  int32_t* d_aux = (int32_t*)ctx->hiAux[ring].p;
  if (hipSetDevice(ctx->device) != hipSuccess ||
      hipMemcpyAsync(d_aux, hm.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, hs) != hipSuccess) { H->fail = 1; return; }
  // sub-chunks: the gather of sub-chunk j + 1 and the scatter of sub-chunk j - 1 run under the host stages of sub-chunk j
  const int SUB = 64;
  const int nsub = (cnt + SUB - 1) / SUB;
  std::vector<hipEvent_t> ev((size_t)nsub, nullptr);
  auto gather = [&](int j) {
    const int j0 = j * SUB, c = std::min(SUB, cnt - j0);
    pipe_copy_bytes_on(hs, c, H->dbuf + (int64_t)j0 * H->dstride, H->dstride, H->pin + (int64_t)j0 * H->pinSlot, H->pinSlot, d_aux + j0, d_aux + cnt + j0);
    if (hipEventCreateWithFlags(&ev[j], hipEventDisableTiming) != hipSuccess || hipEventRecord(ev[j], hs) != hipSuccess) H->fail = 1;
  };
  gather(0);
  for (int j = 0; j < nsub && !H->fail; j++) {
    const int j0 = j * SUB, c = std::min(SUB, cnt - j0);
    if (j + 1 < nsub) gather(j + 1);
    if (H->fail || hipEventSynchronize(ev[j]) != hipSuccess) { H->fail = 1; break; }
    HostInvSub S{H, j0};
    kz_parallel_for(c, KZ_HOST_STAGE_THREADS, host_inverse_block_sub, &S);
    if (H->fail) break;
    for (int b = j0; b < j0 + c; b++) { hm[2 * cnt + b] = H->len[b]; hm[3 * cnt + b] = (hm[cnt + b] && !H->status[b]) ? 1 : 0; }
    if (hipMemcpyAsync(d_aux + 2 * cnt + j0, hm.data() + 2 * cnt + j0, (size_t)c * 4, hipMemcpyHostToDevice, hs) != hipSuccess ||
        hipMemcpyAsync(d_aux + 3 * cnt + j0, hm.data() + 3 * cnt + j0, (size_t)c * 4, hipMemcpyHostToDevice, hs) != hipSuccess) { H->fail = 1; break; }
    pipe_copy_bytes_on(hs, c, H->pin + (int64_t)j0 * H->pinSlot, H->pinSlot, H->dbuf + (int64_t)j0 * H->dstride, H->dstride, d_aux + 2 * cnt + j0, d_aux + 3 * cnt + j0);
  }
  if (hipStreamSynchronize(hs) != hipSuccess) H->fail = 1;
  for (auto e : ev) if (e) hipEventDestroy(e);
}
