// kz_cm.hip -- CM, the context-model binary entropy coder (entropy id 6) on gfx950.
//
// Replaces K/entropy/CMPredictor.java:100-124 (initial state), :136-160 (update), :172-186 (get, the bitstream version >= 4 branch),
// K/entropy/BinaryEntropyEncoder.java:117-155 (encode), :187-204 (encodeBit), :212-218 (flush), :250-255 (dispose) and
// K/entropy/BinaryEntropyDecoder.java:117-167 (decode), :196-218 (decodeBit), :226-239 (read).
//
// The coder is FPAQ's (kz_fpaq.hip): 56-bit low / high, 32-bit flushes, a block is  varint(szBytes) | payload | 56-bit tail  (one
// coder and one fresh predictor per block; blocks below 64 MiB are ONE chunk, longer ones are refused: KZ_CM_MAX_BLOCK).  What is
// new is the predictor: counter1[256][257] and counter2[512][17].  Every counter stays in [0, 65535] (tests/cmmodel.py keeps the
// bounds), so the state is u16: 148 992 bytes, one block's whole predictor in one CU's LDS.  ONE WORKGROUP OF ONE WAVE PER BLOCK; the
// grid is the batch, the hardware queues what is not resident (one workgroup per CU).
//
// Encode: bit k of a byte (7 = first) uses row ctx of counter1 with ctx in [2^(7-k), 2^(8-k)) and row ctx | runMask of counter2; c1, c2
// and runMask come from the input.  The eight tree levels own disjoint rows and none depends on the coder: lane l runs level l & 7
// for every byte (get + update: five LDS reads in two round trips, four writes) and hands the 12-bit prediction over with
// v_readlane; the eight copies of a level compute the same values and store them to the same places, which spares masking lanes
// off.  The low / high chain is wave-uniform (it costs one lane's instructions).  Payload words are held one per lane and leave 64 at a
// time (one 256-byte store) for the block's scratch row; varint, payload and tail go behind the block header when the length is known.
//
// Decode: the row of level k depends on the decoded bits, so the chain is serial: predict (two LDS round trips), decide, update, one
// conditional 32-bit read from a 256-byte window held one word per lane.  Everything is wave-uniform.
//
// LDS banks: a counter1 row is 514 bytes, so the word of column c in row ctx falls on bank ((ctx + c) / 2) mod 32.  The eight levels
// read eight rows (the copies of a level share an address and broadcast): with one column, ctx 1, 64 and 128 can meet on one bank, a
// 3-way conflict at worst, two extra LDS cycles on a ~50-cycle round trip that the step waits for anyway.  Padding rows would not
// buy anything a lone wave could notice.
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_cm_host.h"
#include <algorithm>

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;

#define CM_TOP 0x00FFFFFFFFFFFFFFULL
#define CM_M2456 0x00FFFFFFFF000000ULL
#define CM_M024 0x0000000000FFFFFFULL
#define CM_M032 0x00000000FFFFFFFFULL
#define CM_M056 0x00FFFFFFFFFFFFFFULL
#define CM_PSCALE 65536
#define CM_C1_ROW 257
#define CM_C2_ROW 17
#define CM_C1_SIZE (256 * CM_C1_ROW)
#define CM_C2_SIZE (512 * CM_C2_ROW)

typedef u32 __attribute__((aligned(1))) cm_u32_unaligned;
// a value every lane holds alike, told to the compiler: the chain that uses it stays on the scalar unit
__device__ __forceinline__ u64 cm_uniform64(u64 v) {
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

// CMPredictor.java:100-124: counter1 all PSCALE / 2; counter2[.][j] = j << 12 for j < 16, 65535 for j = 16
__device__ __forceinline__ void cm_init(u16* __restrict__ c1t, u16* __restrict__ c2t, int lane) {
  u32* w = (u32*)c1t;                                              // CM_C1_SIZE is even
  for (int i = lane; i < CM_C1_SIZE / 2; i += 64) w[i] = 0x80008000u;
  for (int i = lane; i < CM_C2_SIZE; i += 64) { const int j = i % CM_C2_ROW; c2t[i] = (u16)(j == 16 ? 65535 : j << 12); }
  __syncthreads();
}

// CMPredictor.update of one counter: c -= (c - (bit ? PSCALE - 16 : 0)) >> rate (arithmetic shift, :141-150); k = bit ? PSCALE - 16 : 0
#define CM_UPD(C, K, RATE) ((C) - (((C) - (K)) >> (RATE)))

// ---- the encoder's output: 32-bit words, big endian, lane (n & 63) holds word n until 64 of them leave with one store ----
struct CmOut { u32* w; u32 cap; u32 n; u32 hold; bool over; };
__device__ __forceinline__ void cm_word(CmOut& o, u32 word, int lane) {
  o.hold = (lane == (int)(o.n & 63u)) ? __builtin_bswap32(word) : o.hold;
  o.n++;
  if ((o.n & 63u) == 0) {                                         // cap is a multiple of 64 words: a row is inside or outside as a whole
    if (o.n <= o.cap) o.w[o.n - 64 + lane] = o.hold; else o.over = true;
  }
}

// One coder step (BinaryEntropyEncoder.java:187-204 encodeBit + :212-218 flush), all operands wave-uniform.  pred <= 4095 and
// (high - low) >> 4 < 2^52: the product fits 64 bits.
#define CM_ENC_BIT(PRED, BIT)                                                                  \
  { const u64 split = (((high - low) >> 4) * (u64)(u32)(PRED)) >> 8;                           \
    if (BIT) high = low + split; else low += split + 1;                                        \
    if (((low ^ high) & CM_M2456) == 0) {            /* never twice in a row: bits 24..31 then differ (00 vs FF) */ \
      cm_word(o, (u32)(high >> 24), lane);                                                     \
      low <<= 32;                                                                              \
      high = (high << 32) | CM_M032;                                                           \
    } }

// rowBytes: what a block may fill of its output row, the block header included
__global__ __launch_bounds__(64) void k_cm_enc(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len,
                                                u8* __restrict__ scr, int64_t scrStride, u8* __restrict__ out, int64_t outStride,
                                                const int32_t* __restrict__ d_hdrBytes, int64_t* __restrict__ d_bits,
                                                int32_t* __restrict__ d_flag, int64_t rowBytes) {
  __shared__ __attribute__((aligned(4))) u16 c1t[CM_C1_SIZE];
  __shared__ u16 c2t[CM_C2_SIZE];
  const int b = blockIdx.x, lane = kz_lane();
  const int count = d_len[b];
  if (lane == 0) d_flag[b] = 1;
  if (count <= 0) { if (lane == 0) d_bits[b] = 0; return; }
  cm_init(c1t, c2t, lane);
  const u8* blk = src + (int64_t)b * stride;
  // the payload buffer goes by the block's own length (kz_cm_payload_cap below; scrStride is that of the longest block): whether a
  // block fits does not depend on its neighbours
  const u32 capWords = (u32)((((int64_t)count + (count >> 3) + 1024 + 255) & ~255LL) >> 2);
  CmOut o{(u32*)(scr + (int64_t)b * scrStride), capWords, 0u, 0u, false};
  u64 low = 0, high = CM_TOP;
  const int sh = 7 - (lane & 7);                                   // this lane's level codes bit sh of every byte
  int c1 = 0, c2 = 0, runMask = 0;                                 // uniform: they follow the input
  for (int row = 0; row < count; row += 64) {
    const int rowCnt = min(64, count - row);
    const u32 rowv = (row + lane < count) ? (u32)blk[row + lane] : 0u;
    for (int j = 0; j < rowCnt; j++) {
      const int val = __builtin_amdgcn_readlane((int)rowv, j);
      // ---- CMPredictor.get (:172-186) and update (:136-160) of this lane's level ----
      const int ctx = (val | 256) >> (sh + 1);
      const int bit = (val >> sh) & 1;
      u16* pc1 = c1t + ctx * CM_C1_ROW;
      const int a = pc1[256], bb = pc1[c1], cc = pc1[c2];
      const int p = (13 * (a + bb) + 6 * cc) >> 5;                 // <= 65535: idx <= 15
      u16* pc2 = c2t + (ctx | runMask) * CM_C2_ROW + (p >> 12);
      const int x1 = pc2[0], x2 = pc2[1];
      const int pred = (p + p + 3 * (x1 + x2) + 64) >> 7;
      const int k = bit ? CM_PSCALE - 16 : 0;
      pc1[256] = (u16)CM_UPD(a, k, 2);                             // FAST_RATE
      pc1[c1] = (u16)CM_UPD(bb, k, 4);                             // MEDIUM_RATE
      pc2[0] = (u16)CM_UPD(x1, k, 6);                              // SLOW_RATE
      pc2[1] = (u16)CM_UPD(x2, k, 6);
      c2 = c1; c1 = val; runMask = (c1 == c2) ? 0x100 : 0;         // :154-159
      // ---- the eight coder steps ----
      const int p7 = __builtin_amdgcn_readlane(pred, 0), p6 = __builtin_amdgcn_readlane(pred, 1), p5 = __builtin_amdgcn_readlane(pred, 2),
                p4 = __builtin_amdgcn_readlane(pred, 3), p3 = __builtin_amdgcn_readlane(pred, 4), p2 = __builtin_amdgcn_readlane(pred, 5),
                p1 = __builtin_amdgcn_readlane(pred, 6), p0 = __builtin_amdgcn_readlane(pred, 7);
      CM_ENC_BIT(p7, val & 0x80) CM_ENC_BIT(p6, val & 0x40) CM_ENC_BIT(p5, val & 0x20) CM_ENC_BIT(p4, val & 0x10)
      CM_ENC_BIT(p3, val & 0x08) CM_ENC_BIT(p2, val & 0x04) CM_ENC_BIT(p1, val & 0x02) CM_ENC_BIT(p0, val & 0x01)
    }
  }
  // the words still held
  if ((o.n & 63u) != 0) {
    if (o.n > o.cap) o.over = true;
    else if ((u32)lane < (o.n & 63u)) o.w[(o.n & ~63u) + (u32)lane] = o.hold;
  }
  // ---- varint(szBytes) | payload | (low | MASK_0_24) as 56 bits (:145-147, dispose :250-255) ----
  const u32 sz = 4u * o.n;
  int vl = 1;
  for (u32 v = sz; v >= 128; v >>= 7) vl++;
  const int hdr = d_hdrBytes[b];
  if (o.over || (int64_t)hdr + vl + (int64_t)sz + 7 > rowBytes) {  // does not fit its row: the block fails, nothing of it is written
    if (lane == 0) { d_flag[b] = 0; d_bits[b] = 0; }
    return;
  }
  u8* op = out + (int64_t)b * outStride + hdr;
  if (lane == 0) { u32 v = sz; int q = 0; while (v >= 128) { op[q++] = (u8)(0x80 | (v & 0x7F)); v >>= 7; } op[q] = (u8)v; }
  __threadfence();                                                 // the scratch row was written by other lanes of this wave
  __syncthreads();
  for (u32 i = (u32)lane; i < o.n; i += 64) *(cm_u32_unaligned*)(op + vl + 4 * (int64_t)i) = o.w[i];
  { const u64 t = low | CM_M024; if (lane < 7) op[vl + (int64_t)sz + lane] = (u8)(t >> (8 * (6 - lane))); }
  if (lane == 0) d_bits[b] = 8LL * (vl + (int64_t)sz + 7);
}

__global__ __launch_bounds__(64) void k_cm_dec(const u8* __restrict__ in, int64_t inStride, const int64_t* __restrict__ d_bitOff,
                                                const int64_t* __restrict__ d_bitEnd, const int32_t* __restrict__ d_len,
                                                u8* __restrict__ dst, int64_t stride, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                long long* __restrict__ endOut) {
  __shared__ __attribute__((aligned(4))) u16 c1t[CM_C1_SIZE];
  __shared__ u16 c2t[CM_C2_SIZE];
  const int b = blockIdx.x, lane = kz_lane();
  const int count = d_len[b];
  if (lane == 0) { d_len2[b] = count; d_flag[b] = 1; }
  if (count <= 0) { if (endOut && lane == 0) endOut[b] = d_bitOff[b]; return; }
  cm_init(c1t, c2t, lane);
  const u8* p = in + (int64_t)b * inStride + (d_bitOff[b] >> 3);  // the payload is byte aligned behind the block header
  const int64_t avail = (d_bitEnd[b] - d_bitOff[b]) >> 3;
  u8* o = dst + (int64_t)b * stride;
  bool bad = ((d_bitOff[b] & 7) != 0);
  int64_t ipos = 0;
  int done = 0;                                                    // bytes stored
  // ---- EntropyUtils.readVarInt; a read past the block's bits throws in the reference ----
  u32 sz = 0;
  if (!bad) {
    if (avail < 1) bad = true;
    else {
      u32 v = p[ipos++]; sz = v & 0x7F; int shift = 7;
      while (v >= 128) {
        if (ipos >= avail) { bad = true; break; }
        v = p[ipos++]; sz |= (v & 0x7F) << shift;
        if (shift == 28) break;
        shift += 7;
      }
    }
  }
  // :141-144 (count < 2^26: count << 5 fits); a negative szBytes fails the payload read; then readBits(56) and the payload
  if (!bad && ((int32_t)sz < 0 || (int64_t)sz > std::min<int64_t>((int64_t)count << 5, 0x7FFFFFFF >> 3) || ipos + 7 + (int64_t)sz > avail)) bad = true;
  if (!bad) {
    u64 current = 0;
    for (int k = 0; k < 7; k++) current = (current << 8) | (u64)p[ipos + k];
    ipos += 7;
    current = cm_uniform64(current);
    const u8* buf = p + ipos;
    const int bufLimit = (int)sz;
    ipos += sz;
    int idx = 0;
    // 256-byte read window (one big-endian word per lane) over the payload; words that reach past bufLimit are never taken
    int wbase = 0;
    u32 win = (4 * lane + 4 <= bufLimit) ? __builtin_bswap32(*(const cm_u32_unaligned*)(buf + 4 * lane)) : 0u;
    u64 low = 0, high = CM_TOP;
    int c1 = 0, c2 = 0, runMask = 0;
    for (int row = 0; row < count && !bad; row += 64) {
      const int rowCnt = min(64, count - row);
      u32 outv = 0;
      for (int j = 0; j < rowCnt; j++) {
        int ctx = 1;
#pragma unroll
        for (int level = 0; level < 8; level++) {
          // CMPredictor.get (:172-186)
          u16* pc1 = c1t + ctx * CM_C1_ROW;
          const int a = pc1[256], bb = pc1[c1], cc = pc1[c2];
          const int pp = (13 * (a + bb) + 6 * cc) >> 5;
          u16* pc2 = c2t + (ctx | runMask) * CM_C2_ROW + (pp >> 12);
          const int x1 = pc2[0], x2 = pc2[1];
          const u32 pred = (u32)__builtin_amdgcn_readfirstlane((pp + pp + 3 * (x1 + x2) + 64) >> 7);
          // decodeBit (:196-218)
          const u64 split = ((((high - low) >> 4) * (u64)pred) >> 8) + low;
          const bool one = split >= current;
          if (one) high = split; else low = split + 1;
          const int k = one ? CM_PSCALE - 16 : 0;
          pc1[256] = (u16)CM_UPD(a, k, 2);
          pc1[c1] = (u16)CM_UPD(bb, k, 4);
          pc2[0] = (u16)CM_UPD(x1, k, 6);
          pc2[1] = (u16)CM_UPD(x2, k, 6);
          ctx = ctx + ctx + (one ? 1 : 0);
          if (((low ^ high) & CM_M2456) == 0) {                    // read (:226-239); never twice in a row, as in the encoder
            low = (low << 32) & CM_M056;
            high = ((high << 32) | CM_M032) & CM_M056;
            if (idx + 4 > bufLimit) { current = (current << 32) & CM_M056; idx = bufLimit + 1; }
            else {
              if (idx >= wbase + 256) {
                wbase = idx;
                win = (wbase + 4 * lane + 4 <= bufLimit) ? __builtin_bswap32(*(const cm_u32_unaligned*)(buf + wbase + 4 * lane)) : 0u;
              }
              const u64 w = (u64)(u32)__builtin_amdgcn_readlane((int)win, (idx - wbase) >> 2);
              current = ((current << 32) | w) & CM_M056;
              idx += 4;
            }
          }
        }
        const int val = ctx & 0xFF;
        outv = (lane == j) ? (u32)val : outv;
        c2 = c1; c1 = val; runMask = (c1 == c2) ? 0x100 : 0;
        if (idx > bufLimit) { bad = true; break; }                 // :159-160: the block fails behind the byte in which a read ran dry
      }
      if (!bad) { if (lane < rowCnt) o[row + lane] = (u8)outv; done = row + rowCnt; }
    }
  }
  if (bad) {                                                       // what was not decoded is zero, as the other decoders leave it
    for (int i = done + lane; i < count; i += 64) o[i] = 0;
    if (lane == 0) d_flag[b] = 0;
  }
  if (endOut && lane == 0) endOut[b] = (long long)(d_bitOff[b] + 8LL * ipos);   // bits consumed (EntropyDecoder contract)
}

size_t kz_cm_scratch(int B, int maxN, bool decode) {
  if (decode) return 4096;
  return (size_t)B * (size_t)kz_cm_payload_cap(maxN) + 4096;
}

static int cm_check_lengths(kz_ctx* ctx, const kz_batch& bt, const char* what) {
  for (int b = 0; b < bt.B; b++)
    if (bt.h_len[b] >= KZ_CM_MAX_BLOCK) {
      snprintf(ctx->err, sizeof(ctx->err), "cm %s: block of %d bytes: CM blocks go up to (1 << 26) - 1 bytes (the reference codes longer ones in chunks)", what, bt.h_len[b]);
      return -KZ_ERR_INVALID_CODEC;
    }
  return 0;
}

int kz_stage_cm_encode(kz_ctx* ctx, kz_batch& bt, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits) {
  const int B = bt.B;
  { const int rc = cm_check_lengths(ctx, bt, "encode"); if (rc) return rc; }
  int maxN = 0;
  for (int b = 0; b < B; b++) maxN = std::max(maxN, bt.h_len[b]);
  const int64_t scrStride = kz_cm_payload_cap(maxN);
  u8* scr = (u8*)kz_arena_alloc(ctx, (size_t)scrStride * B);
  if (!scr) { snprintf(ctx->err, sizeof(ctx->err), "cm encode: arena overflow"); return -KZ_ERR_DEVICE; }
  // KZ_CM_TEST_ROW_BYTES (tests): a row shorter than the stride, to reach the bound check with blocks of test size
  const int64_t rowBytes = (ctx->sw.cmTestRowBytes > 0) ? std::min<int64_t>(outStride, ctx->sw.cmTestRowBytes) : outStride;
  KZ_LAUNCH(ctx, KID_CM_ENC, k_cm_enc, dim3(B), dim3(64), bt.buf[bt.cur], bt.stride, bt.d_len, scr, scrStride, out, outStride, d_hdrBytes, d_bits, bt.d_flag, rowBytes);
  KZ_HIP(hipGetLastError());
  return 0;
}

int kz_stage_cm_decode(kz_ctx* ctx, kz_batch& bt, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd) {
  const int B = bt.B;
  { const int rc = cm_check_lengths(ctx, bt, "decode"); if (rc) return rc; }
  u8* dst = bt.buf[bt.cur ^ 1];
  KZ_LAUNCH(ctx, KID_CM_DEC, k_cm_dec, dim3(B), dim3(64), in, inStride, d_bitOff, d_bitEnd, bt.d_len, dst, bt.stride, bt.d_len2, bt.d_flag, ctx->d_endBits);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
