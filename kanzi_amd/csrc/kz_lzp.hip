// kz_lzp.hip -- LZP (LZCodec.LZPCodec, transform id 14) on gfx950, bitstream 7 (minMatch 64).
//
// Replaces K/transform/LZCodec.java:1023-1133 (forward), :1145-1244 (inverse), :1257-1273 (findMatch).
//
// LZP predicts ONE candidate per position from a hash of the four preceding bytes (2^16 ints, last writer wins) and codes a match
// of at least 64 bytes as 0xFC + length; every other position is a literal (a literal 0xFC whose table entry is set is followed by
// 0xFF).  The parse is serial in the table, but at a literal the hash needs only source bytes (forward) or bytes already decoded
// (inverse) and at most three carried bytes.  So one wave per block parses in speculative WINDOWS of 64 positions: lane j takes
// position s + j and assumes that everything before it in the window is a plain literal.  The first lane that turns out to be
// something else (a match; in the inverse a 0xFC with a set entry) ends the window; only the lanes up to it are committed.  The
// hash table lives in the context's arena (256 KiB per block: more than a CU's LDS) and is zeroed by the kernel for every block.
//
// ctx changes byte order (:1061, :1081, :1095): it starts, and restarts after a match, as the LITTLE-endian read of the last four
// bytes, and every literal shifts one byte in from the right, so after four literals it is their BIG-endian value.  Lane j < 4 of a
// window therefore builds (carried ctx << 8j) | (the j bytes since), lanes j >= 4 the big-endian value of their own last four bytes.
#include "kz_device.h"
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "k_lzp_fwd / k_lzp_inv rely on the in-order store -> load visibility of one wave on gfx9 / CDNA: see the note at k_lz_inv's match copy"
#endif
#include "kz_internal.h"

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint8_t u8;

// one wave per block: its vector memory operations are performed in program order, only the compiler has to be told (kz_lz.hip)
#define LZP_ORDER() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define LZP_SEED 0x7FEB352Du
#define LZP_HASH_LOG 16
#define LZP_MIN_MATCH 64
#define LZP_MIN_BLOCK 128
#define LZP_FLAG 0xFC
#define LZP_WINDOW 64            // positions per speculative window = lanes of the wave
#define LZP_TAGS 1024            // LDS slots of the duplicate-hash test

typedef u64 __attribute__((aligned(1))) lzp_u64_unaligned;
typedef u32 __attribute__((aligned(1))) lzp_u32_unaligned;
__device__ __forceinline__ u64 lzp_le64(const u8* p) { return *(const lzp_u64_unaligned*)p; }
__device__ __forceinline__ u32 lzp_le32(const u8* p) { return *(const lzp_u32_unaligned*)p; }
__device__ __forceinline__ u32 lzp_hash(u32 ctx) { return (LZP_SEED * ctx) >> (32 - LZP_HASH_LOG); }
// ctx of the position j literals behind the one whose ctx is `carried`; be4 = big-endian value of the four bytes before it
__device__ __forceinline__ u32 lzp_ctx(u32 carried, int j, u32 be4) {
  if (j >= 4) return be4;
  if (j == 0) return carried;
  const u32 m = (1u << (8 * j)) - 1u;
  return (carried << (8 * j)) | (be4 & m);
}
// findMatch (:1257-1273): 8 bytes per step, cut to whole steps at maxMatch; the wave compares 512 bytes per round trip.  All
// arguments are wave-uniform.  Loads stay below srcIdx + maxMatch.
__device__ __forceinline__ int lzp_find_match(const u8* src, int srcIdx, int ref, int maxMatch) {
  const int lane = kz_lane();
  int bestLen = 0;
  while (bestLen + 8 <= maxMatch) {
    const int off = bestLen + 8 * lane;
    const bool in = off + 8 <= maxMatch;
    const u64 diff = in ? (lzp_le64(src + srcIdx + off) ^ lzp_le64(src + ref + off)) : 0ULL;
    const uint64_t inMask = kz_ballot(in);
    const uint64_t dm = kz_ballot(in && diff != 0);
    if (dm) {
      const int l = (int)__builtin_ctzll(dm);
      const u32 dlo = (u32)__builtin_amdgcn_readlane((int)(u32)diff, l), dhi = (u32)__builtin_amdgcn_readlane((int)(u32)(diff >> 32), l);
      const u64 dd = ((u64)dhi << 32) | dlo;
      return bestLen + 8 * l + (int)(__builtin_ctzll(dd) >> 3);
    }
    bestLen += 8 * (int)__builtin_popcountll(inMask);
  }
  return bestLen;
}

// The table entries the lanes of a window would read if the positions before them were visited in order: hashes[h], or, where an
// earlier lane of the window has the same hash, that lane's position (posBase + its lane).  `peers` = the valid lanes that share
// this lane's hash (itself included).  Duplicates are looked for with one LDS slot per 10-bit hash fragment: every lane writes its
// number and reads the slot back; equal hashes share a slot, so a window in which every lane reads its own number has none.  Only
// otherwise the lanes are matched on all 16 bits (runs make every lane of a window collide: this path is taken often, then).
__device__ __forceinline__ int lzp_window_refs(const int32_t* hashes, u32 h, bool valid, int posBase, uint16_t* tags, uint64_t& peers) {
  const int lane = kz_lane();
  if (valid) tags[h & (LZP_TAGS - 1)] = (uint16_t)lane;
  __syncthreads();                                                   // one wave: orders the LDS write and read, no other wave waits
  const bool dup = valid && tags[h & (LZP_TAGS - 1)] != (uint16_t)lane;
  int ref = valid ? hashes[h] : 0;
  peers = valid ? (1ULL << lane) : 0ULL;
  if (kz_ballot(dup)) {
    uint64_t m = kz_ballot(valid);
#pragma unroll
    for (int bb = 0; bb < LZP_HASH_LOG; bb++) {
      const uint64_t bal = kz_ballot(((h >> bb) & 1u) != 0u);
      m &= ((h >> bb) & 1u) ? bal : ~bal;
    }
    peers = valid ? m : 0ULL;
    const uint64_t earlier = peers & kz_lanemask_lt();
    if (earlier) ref = posBase + 63 - (int)__builtin_clzll(earlier);
  }
  __syncthreads();                                                   // the next window's writes stay behind this one's reads
  return ref;
}
// the committed lanes store their positions; of equal hashes the highest position wins, as it would in order
__device__ __forceinline__ void lzp_window_store(int32_t* hashes, u32 h, int pos, uint64_t peers, uint64_t committed) {
  const int lane = kz_lane();
  const uint64_t self = 1ULL << lane;
  const uint64_t later = peers & committed & ~(kz_lanemask_lt() | self);
  if ((committed & self) && later == 0) hashes[h] = pos;
}
__device__ __forceinline__ void lzp_zero_table(int32_t* hashes) {
  int4* t = (int4*)hashes;
  const int4 z = make_int4(0, 0, 0, 0);
  for (int i = (int)threadIdx.x; i < (1 << LZP_HASH_LOG) / 4; i += (int)blockDim.x) t[i] = z;
}

__global__ __launch_bounds__(64) void k_lzp_fwd(const u8* __restrict__ srcAll, u8* __restrict__ dstAll, int64_t stride,
                                                const int32_t* __restrict__ d_len, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                int32_t* __restrict__ hashAll) {
  __shared__ uint16_t tags[LZP_TAGS];
  const int b = blockIdx.x;
  const int count = __builtin_amdgcn_readfirstlane(d_len[b]);
  const int lane = kz_lane();
  const u8* src = srcAll + (int64_t)b * stride;
  u8* dst = dstAll + (int64_t)b * stride;
  if (count < LZP_MIN_BLOCK) { if (lane == 0) { d_len2[b] = count; d_flag[b] = 0; } return; }     // :1038-1039 (count == 0: the caller)
  int32_t* hashes = hashAll + ((int64_t)b << LZP_HASH_LOG);
  lzp_zero_table(hashes);
  const int srcEnd = count;
  const int dstEnd = count - (count >> 6);                           // :1053
  const int matchEnd = srcEnd - LZP_MIN_MATCH;                       // positions below it may start a match (:1066); the others: :1114-1128
  if (lane < 4) dst[lane] = src[lane];                               // :1057-1060
  u32 ctx = lzp_le32(src);                                           // :1061
  int srcIdx = 4, dstIdx = 4;
  LZP_ORDER();
  // dstIdx only grows and the verdict asks for dstIdx < dstEnd at the end (:1132); every `return false` on the way is a dstIdx that
  // has reached dstEnd (:1085, :1104-1109) and both loops stop there too.  So the block declines as soon as dstIdx >= dstEnd, and
  // stores are kept below dstEnd.
  while (srcIdx < srcEnd && dstIdx < dstEnd) {
    const int p = srcIdx + lane;
    const bool valid = p < srcEnd;
    // bytes p-4 .. p+3 (p >= 4; reads past the block's end stay inside its slot and are not used)
    const u64 around = valid ? lzp_le64(src + p - 4) : 0ULL;
    const u32 be4 = __builtin_bswap32((u32)around);
    const u32 val = (u32)(around >> 32) & 0xFFu;
    const u32 h = lzp_hash(lzp_ctx(ctx, lane, be4));
    uint64_t peers;
    const int ref = lzp_window_refs(hashes, h, valid, srcIdx, tags, peers);
    // candidates (:1073-1074): the int compare at +60 is only a shortcut for "not 64 equal bytes"
    bool cand = valid && p < matchEnd && ref != 0;
    if (cand) cand = lzp_le32(src + ref + LZP_MIN_MATCH - 4) == lzp_le32(src + p + LZP_MIN_MATCH - 4);
    int F = min(LZP_WINDOW, srcEnd - srcIdx);                       // lanes below F are literals
    int bestLen = 0;
    for (uint64_t cm = kz_ballot(cand); cm; cm &= cm - 1) {
      const int l = (int)__builtin_ctzll(cm);
      const int len = lzp_find_match(src, srcIdx + l, __builtin_amdgcn_readlane(ref, l), srcEnd - (srcIdx + l));
      if (len >= LZP_MIN_MATCH) { F = l; bestLen = len; break; }     // shorter: the literal it was assumed to be
    }
    const bool isMatch = bestLen != 0;
    const uint64_t lits = (F >= 64) ? ~0ULL : ((1ULL << F) - 1ULL);
    lzp_window_store(hashes, h, p, peers, isMatch ? (lits | (1ULL << F)) : lits);     // the match position is visited too (:1069)
    // literals and escapes (:1080-1089)
    const bool isLit = lane < F;
    const bool esc = isLit && val == LZP_FLAG && ref != 0;
    const uint64_t em = kz_ballot(esc);
    const int o = dstIdx + lane + (int)__builtin_popcountll(em & kz_lanemask_lt());
    if (isLit && o < dstEnd) dst[o] = (u8)val;
    if (esc && o + 1 < dstEnd) dst[o + 1] = 0xFF;
    dstIdx += F + (int)__builtin_popcountll(em);
    if (!isMatch) {
      // F literals on: the ctx lane F would have built
      const u32 beF = __builtin_bswap32(lzp_le32(src + srcIdx + F - 4));
      ctx = lzp_ctx(ctx, F, beF);
      srcIdx += F;
      LZP_ORDER();
      continue;
    }
    if (dstIdx >= dstEnd) break;                                     // :1066 at the match position
    srcIdx += F + bestLen;                                           // :1094-1111
    ctx = lzp_le32(src + srcIdx - 4);
    const int extra = bestLen - LZP_MIN_MATCH;
    const int nFE = extra / 254;
    if (lane == 0) dst[dstIdx] = LZP_FLAG;
    dstIdx++;
    for (int i = lane; i < nFE && dstIdx + i < dstEnd; i += 64) dst[dstIdx + i] = 0xFE;
    dstIdx += nFE;
    if (dstIdx >= dstEnd) break;                                     // :1104-1109
    if (lane == 0) dst[dstIdx] = (u8)(extra - nFE * 254);
    dstIdx++;
    LZP_ORDER();
  }
  const bool ok = srcIdx == srcEnd && dstIdx < dstEnd;               // :1132
  if (lane == 0) { d_flag[b] = ok ? 1 : 0; d_len2[b] = ok ? dstIdx : count; }
}

__global__ __launch_bounds__(64) void k_lzp_inv(const u8* __restrict__ srcAll, u8* __restrict__ dstAll, int64_t stride,
                                                const int32_t* __restrict__ d_len, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                int32_t* __restrict__ hashAll, int dstCap) {
  __shared__ uint16_t tags[LZP_TAGS];
  const int b = blockIdx.x;
  const int count = __builtin_amdgcn_readfirstlane(d_len[b]);
  const int lane = kz_lane();
  const u8* src = srcAll + (int64_t)b * stride;
  u8* dst = dstAll + (int64_t)b * stride;
  if (count == 0) { if (lane == 0) { d_len2[b] = 0; d_flag[b] = 1; } return; }                  // :1146-1147
  // :1163-1164; fewer than 4 bytes: the first reads (:1173-1176) leave srcIdx = 4 behind srcEnd (or throw)
  if (dstCap < count || count < 4) { if (lane == 0) { d_len2[b] = 0; d_flag[b] = 0; } return; }
  int32_t* hashes = hashAll + ((int64_t)b << LZP_HASH_LOG);
  lzp_zero_table(hashes);
  const int srcEnd = count;
  const int dstEnd = dstCap;                                         // :1158
  if (lane < 4) dst[lane] = src[lane];
  u32 ctx = lzp_le32(src);                                           // :1177
  int srcIdx = 4, dstIdx = 4;
  bool ok = true;
  LZP_ORDER();
  while (srcIdx < srcEnd) {
    // lane j takes src[srcIdx + j] for the plain literal that lands at dstIdx + j: the four bytes in front of it are then the
    // four source bytes in front of it (for j < 4 the carried ctx stands in for those in front of the window)
    const int p = srcIdx + lane;
    const bool valid = p < srcEnd;
    const u64 around = valid ? lzp_le64(src + p - 4) : 0ULL;
    const u32 be4 = __builtin_bswap32((u32)around);
    const u32 val = (u32)(around >> 32) & 0xFFu;
    const u32 myCtx = lzp_ctx(ctx, lane, be4);
    const u32 h = lzp_hash(myCtx);
    uint64_t peers;
    const int ref = lzp_window_refs(hashes, h, valid, dstIdx, tags, peers);
    const uint64_t sm = kz_ballot(valid && val == LZP_FLAG && ref != 0);       // :1186
    const int nv = min(LZP_WINDOW, srcEnd - srcIdx);
    const int F = sm ? (int)__builtin_ctzll(sm) : nv;
    const uint64_t lits = (F >= 64) ? ~0ULL : ((1ULL << F) - 1ULL);
    lzp_window_store(hashes, h, dstIdx + lane, peers, sm ? (lits | (1ULL << F)) : lits);   // :1184
    if (lane < F && dstIdx + lane < dstEnd) dst[dstIdx + lane] = (u8)val;
    if (dstIdx + F > dstEnd) { ok = false; break; }                  // :1187-1188
    if (!sm) {
      const u32 beF = __builtin_bswap32(lzp_le32(src + srcIdx + F - 4));
      ctx = lzp_ctx(ctx, F, beF);
      srcIdx += F; dstIdx += F;
      LZP_ORDER();
      continue;
    }
    const u32 ctxF = (u32)__builtin_amdgcn_readlane((int)myCtx, F);
    const int refF = __builtin_amdgcn_readlane(ref, F);
    srcIdx += F + 1; dstIdx += F;
    if (srcIdx >= srcEnd) { ok = false; break; }                     // :1199-1200
    const u32 c = (u32)__builtin_amdgcn_readfirstlane((int)src[srcIdx]);
    if (c == 0xFF) {                                                 // :1202-1211
      if (dstIdx >= dstEnd) { ok = false; break; }
      if (lane == 0) dst[dstIdx] = LZP_FLAG;
      ctx = (ctxF << 8) | LZP_FLAG;
      srcIdx++; dstIdx++;
      LZP_ORDER();
      continue;
    }
    // the length (:1213-1225), in 64 bits: the reference's int wraps behind 8 MiB of 0xFE bytes
    long long mLen = LZP_MIN_MATCH;
    for (;;) {
      const int q = srcIdx + lane;
      const uint64_t notFE = kz_ballot(q >= srcEnd || src[q] != 0xFE);
      const int n = notFE ? (int)__builtin_ctzll(notFE) : 64;
      srcIdx += n; mLen += 254LL * n;
      if (notFE) break;
    }
    if (srcIdx >= srcEnd) { ok = false; break; }                     // :1221-1222 (without a 0xFE, :1199 has said so already)
    mLen += __builtin_amdgcn_readfirstlane((int)src[srcIdx]); srcIdx++;
    if ((long long)dstIdx + mLen > (long long)dstEnd) { ok = false; break; }   // :1227-1228
    const int n = (int)mLen;
    const int dist = dstIdx - refF;                                  // > 0: the entry was stored at an earlier position (>= 4)
    // the literals stored above and every earlier store of this wave are visible to the loads below in program order (k_lz_inv)
    LZP_ORDER();
    if (dist >= 64) {
      for (int k = 0; k < n; k += 64) { const int i = k + lane; u8 v = 0; if (i < n) v = dst[refF + i]; LZP_ORDER(); if (i < n) dst[dstIdx + i] = v; LZP_ORDER(); }
    } else {
      // :1232-1235: the source runs into the destination, the output is periodic with period dist over bytes already written
      for (int i = lane; i < n; i += 64) dst[dstIdx + i] = dst[refF + (i % dist)];
    }
    LZP_ORDER();
    dstIdx += n;
    ctx = lzp_le32(dst + dstIdx - 4);                                // :1238
    LZP_ORDER();
  }
  if (ok) ok = srcIdx == srcEnd;                                     // :1243
  if (lane == 0) { d_flag[b] = ok ? 1 : 0; d_len2[b] = ok ? dstIdx : 0; }
}

size_t kz_lzp_scratch(int B, int maxN) {
  (void)maxN;
  return (size_t)B * ((size_t)4 << LZP_HASH_LOG) + 4096;
}

int kz_stage_lzp_forward(kz_ctx* ctx, kz_batch& bt) {
  const int B = bt.B;
  int32_t* hashes = (int32_t*)kz_arena_alloc(ctx, (size_t)B * ((size_t)4 << LZP_HASH_LOG));
  if (!hashes) { snprintf(ctx->err, sizeof(ctx->err), "lzp_forward: arena overflow"); return -KZ_ERR_DEVICE; }
  KZ_LAUNCH(ctx, KID_LZP_FWD, k_lzp_fwd, dim3(B), dim3(64), bt.buf[bt.cur], bt.buf[bt.cur ^ 1], bt.stride, bt.d_len, bt.d_len2, bt.d_flag, hashes);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}

int kz_stage_lzp_inverse(kz_ctx* ctx, kz_batch& bt, int dstCap) {
  const int B = bt.B;
  if ((int64_t)dstCap > bt.stride) dstCap = (int)bt.stride;
  int32_t* hashes = (int32_t*)kz_arena_alloc(ctx, (size_t)B * ((size_t)4 << LZP_HASH_LOG));
  if (!hashes) { snprintf(ctx->err, sizeof(ctx->err), "lzp_inverse: arena overflow"); return -KZ_ERR_DEVICE; }
  KZ_LAUNCH(ctx, KID_LZP_INV, k_lzp_inv, dim3(B), dim3(64), bt.buf[bt.cur], bt.buf[bt.cur ^ 1], bt.stride, bt.d_len, bt.d_len2, bt.d_flag, hashes, dstCap);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
