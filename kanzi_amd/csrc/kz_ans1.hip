// kz_ans1.hip -- order-1 range ANS (ANS1) block encoder / decoder for gfx950.
//
// Replaces K/entropy/ANSRangeEncoder.java (order 1: the (obs, ctx, 1) constructor :154-156 -- logRange 11, chunks of
// 16 KiB << 8 = 4 MiB), encode :263-305, rebuildStatistics :419-449 (Global.computeHistogramOrder1, K/Global.java:341-390),
// updateFrequencies :164-200, encodeHeader :211-252, encodeChunk order-1 branch :359-390, encodeSymbol :315-328,
// Symbol.reset :473-496; K/entropy/EntropyUtils.java:141-250 (normalizeFrequencies, 64-bit product), :38-75 (encodeAlphabet);
// K/entropy/ANSRangeDecoder.java:188-236 (decode), :357-440 (decodeChunkV2, order-1 branch :406-432), :452-544 (decodeHeader).
//
// A chunk is 4 MiB, so a block has one chunk up to 4 MiB and a few beyond.  The coder's state is 256 contexts x 256 symbols per
// chunk: it lives in HBM, one 256 KiB table per chunk.
//   encode: k_ans1_hist (LDS histograms of 64 contexts per workgroup, flushed with global atomics) -> k_ans1_norm (one wave per
//           (chunk, context): normalisation, the context's header length) -> k_ans1_hdr (one workgroup per chunk: scan of the
//           256 header lengths, every context writes its own bits) -> k_ans1_enc (one wave per chunk, lanes 0-3 = st0..st3, the
//           shared output cursor from a 4-lane ballot prefix as in kz_ans.hip) -> k_ans_enc_scan / k_ans_enc_concat (kz_ans.hip).
//   decode: k_ans1_dec_index (one lane per block walks and validates the chunk headers) -> k_ans1_dec_table (one wave per (chunk,
//           context): symbol records + a 2^lr-entry slot table in HBM) -> k_ans1_dec_chunk (one wave per chunk, lanes 0-3 =
//           st3..st0) -> k_ans1_dec_fin (verdict of the lowest chunk with an event, as k_ans_dec_fin).
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_chunk.h"

typedef uint16_t u16;

#define A1_TOP (1u << 15)
#define A1_LR 11                                  // ANSRangeEncoder.java:154 (DEFAULT_LOG_RANGE - 1)
#define A1_CHUNK (1 << 22)                        // :155-156
#define A1_MAX_CHUNK_SIZE (1u << 27)
#define A1_HDR_BYTES 102400                       // 3 + 256 x 3 184 bits: the longest context header is a 255-symbol alphabet
#define A1_SEG (256 * 1024)                       // bytes of a chunk one histogram workgroup reads
#define A1_FAST_LR 11                             // slot tables are built for lr <= 11 (what the encoder writes)
#define A1_RESERVE 32                             // bytes kept in front of a chunk's payload for varint + four states

typedef u16 __attribute__((aligned(1))) a1_u16_unaligned;
typedef u64 __attribute__((aligned(1))) a1_u64_unaligned;

// =================================================================================================
// encode
struct Ans1Enc {
  u32* tab;          // [B][C][256 ctx][256 sym]: counts, then {freq | cum << 16} of the normalised context
  u32* ctxBits;      // [B][C][256] header bits of each context
};

// Global.computeHistogramOrder1 on each quarter: one walk per quarter starting in context 0 (the four interleaved walks of a
// range of 32 bytes or more chain up: prv1 = block[n1 - 1], ...); a chunk of fewer than 4 bytes is a single walk over all of it,
// otherwise the len & 3 tail bytes are not counted.  Workgroup (seg, g): bytes [seg * A1_SEG, +A1_SEG) of the chunk, contexts
// [64 g, 64 g + 64) in a 64 KiB LDS histogram.
__global__ __launch_bounds__(KZ_WG) void k_ans1_hist(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, Ans1Enc A, int C) {
  const int b = blockIdx.z, ck = blockIdx.y, seg = blockIdx.x >> 2, g = blockIdx.x & 3;
  const int count = d_len[b];
  if (count <= 32) return;
  const int start = ck * A1_CHUNK;
  if (start >= count) return;
  const int len = min(count - start, A1_CHUNK);
  const int quarter = len >> 2;
  const int cnt = quarter ? 4 * quarter : len;
  const int s0 = seg * A1_SEG;
  if (s0 >= cnt) return;
  const int s1 = min(cnt, s0 + A1_SEG);
  const u8* data = src + (int64_t)b * stride + start;
  __shared__ u32 hist[64 * 256];
  for (int i = threadIdx.x; i < 64 * 256; i += KZ_WG) hist[i] = 0;
  __syncthreads();
  for (int i0 = s0 + 4 * (int)threadIdx.x; i0 < s1; i0 += 4 * KZ_WG) {
    u32 w;
    if (i0 + 4 <= len) w = *(const u32*)(data + i0);                     // chunk starts are 4 MiB apart in 256-byte aligned slots
    else { w = 0; for (int k = 0; k < 4 && i0 + k < len; k++) w |= (u32)data[i0 + k] << (8 * k); }
    u32 prv = i0 > 0 ? data[i0 - 1] : 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = i0 + k;
      const u32 c = (w >> (8 * k)) & 0xFFu;
      const bool qs = i == 0 || (quarter && (i == quarter || i == 2 * quarter || i == 3 * quarter));
      const u32 ctx = qs ? 0u : prv;
      if (i < s1 && (int)(ctx >> 6) == g) atomicAdd(&hist[((ctx & 63) << 8) | c], 1u);
      prv = c;
    }
  }
  __syncthreads();
  u32* t = A.tab + ((int64_t)b * C + ck) * 65536 + (g << 14);
  for (int i = threadIdx.x; i < 64 * 256; i += KZ_WG) { const u32 v = hist[i]; if (v) atomicAdd(&t[i], v); }
}

// normalizeFrequencies(freqs[ctx], alphabet, total, 2048) (EntropyUtils.java:141-250) for one context, as k_ans_enc_chunk does it
// for ANS0 but with the 64-bit product of :177-178 (a context's total reaches 2^22); then {freq | cum << 16} and the context's
// header length (encodeAlphabet :38-75 + encodeHeader :221-250).
__global__ __launch_bounds__(64) void k_ans1_norm(const int32_t* __restrict__ d_len, Ans1Enc A, int C) {
  const int b = blockIdx.z, ck = blockIdx.y, k = blockIdx.x;
  const int count = d_len[b];
  if (count <= 32 || ck * A1_CHUNK >= count) return;
  const int lane = kz_lane();
  const int64_t ci = (int64_t)b * C + ck;
  u32* t = A.tab + ci * 65536 + (k << 8);
  __shared__ u16 nfreq[256];
  __shared__ u8 alpha[256];
  const u32 scale = 1u << A1_LR;
  u32 f[4]; bool present[4]; u32 alphabetSize = 0;
  u32 total = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    f[q] = t[q * 64 + lane];
    present[q] = f[q] != 0;
    const uint64_t bal = kz_ballot(present[q]);
    if (present[q]) alpha[alphabetSize + (u32)__popcll(bal & kz_lanemask_lt())] = (u8)(q * 64 + lane);
    alphabetSize += (u32)__popcll(bal);
    total += kz_wave_sum(f[q]);
  }
  if (total != 0 && total != scale) {                                       // :155-162 shortcut otherwise
    u32 sumScaled = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (present[q]) {
        const u64 sf = (u64)f[q] * scale;
        f[q] = (sf <= total) ? 1u : (u32)((sf + (total >> 1)) / total);
      }
      sumScaled += kz_wave_sum(present[q] ? f[q] : 0);
    }
    if (alphabetSize == 1) {
#pragma unroll
      for (int q = 0; q < 4; q++) if (present[q]) f[q] = scale;
    } else if (sumScaled != scale) {
      u32 best = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) { u32 v = present[q] ? f[q] : 0; best = max(best, v); }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) best = max(best, (u32)__shfl_xor(best, d, 64));
      int idxMax = 256;                                                      // first symbol holding the maximum (:184-185)
#pragma unroll
      for (int q = 3; q >= 0; q--) {
        const uint64_t bal = kz_ballot(present[q] && f[q] == best);
        if (bal) idxMax = q * 64 + (int)__builtin_ctzll(bal);
      }
      int delta = (int)sumScaled - (int)scale;
      const int errThr = (int)(best >> 4);
      const int mq = idxMax >> 6, ml = idxMax & 63;
      const int ad = delta < 0 ? -delta : delta;
      if (ad <= errThr) {                                                   // :204-208
#pragma unroll
        for (int q = 0; q < 4; q++) if (q == mq && lane == ml) f[q] = (u32)((int)f[q] - delta);
      } else {
        int adj;
        if (delta < 0) { delta += errThr; adj = errThr; } else { delta -= errThr; adj = -errThr; }
#pragma unroll
        for (int q = 0; q < 4; q++) if (q == mq && lane == ml) f[q] = (u32)((int)f[q] + adj);
        const int inc = (delta > 0) ? -1 : 1;                                // :219-246
        delta = delta < 0 ? -delta : delta;
        int round = 0;
        while ((++round < 6) && (delta > 0)) {
          int adjustments = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const bool elig = present[q] && f[q] > 2;
            const uint64_t bal = kz_ballot(elig);
            const int pre = (int)__popcll(bal & kz_lanemask_lt());
            const int tot = (int)__popcll(bal);
            if (elig && pre < delta) f[q] = (u32)((int)f[q] + inc);
            const int used = tot < delta ? tot : delta;
            adjustments += used; delta -= used;
          }
          if (adjustments == 0) break;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) if (q == mq && lane == ml) { int v = (int)f[q] - delta; f[q] = (u32)(v > 1 ? v : 1); }
      }
    }
  }
  u32 cum = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const u32 fv = present[q] ? f[q] : 0;
    const u32 inc = kz_wave_incl_sum(fv);
    const u32 cumFreq = cum + inc - fv;
    cum += __shfl(inc, 63, 64);
    nfreq[q * 64 + lane] = (u16)fv;
    t[q * 64 + lane] = present[q] ? (fv | (cumFreq << 16)) : 0u;
  }
  __syncthreads();
  if (lane == 0) {
    u32 bits;
    if (alphabetSize == 0 || alphabetSize == 256) bits = 2;
    else bits = 6 + 8 * (u32)((alpha[alphabetSize - 1] >> 3) + 1);
    if (alphabetSize > 1) {
      const int chkSize = (alphabetSize >= 64) ? 8 : 6;
      int llr = 3;
      while ((1 << llr) <= A1_LR) llr++;
      for (int i = 1; i < (int)alphabetSize; i += chkSize) {
        const int endj = min(i + chkSize, (int)alphabetSize);
        int mx = 0;
        for (int j = i; j < endj; j++) mx = max(mx, (int)nfreq[alpha[j]] - 1);
        int logMax = 0;
        while ((1 << logMax) <= mx) logMax++;
        bits += llr + logMax * (endj - i);
      }
    }
    A.ctxBits[ci * 256 + k] = bits;
  }
}

// MSB-first bits into a zeroed byte buffer that other threads write too (their bits share boundary bytes)
__device__ __forceinline__ void a1_put(u32* w, u64& pos, u32 v, int count) {
  while (count > 0) {
    const int bitoff = (int)(pos & 7), room = 8 - bitoff;
    const int take = count < room ? count : room;
    const u32 bits = (v >> (count - take)) & ((1u << take) - 1u);
    const u64 by = pos >> 3;
    atomicOr(&w[by >> 2], (bits << (room - take)) << (8 * (u32)(by & 3)));
    pos += take; count -= take;
  }
}

// header of one chunk: lr - 8 (3 bits), then every context's alphabet and frequency chunks at the offset the scan gives it
__global__ __launch_bounds__(256) void k_ans1_hdr(const int32_t* __restrict__ d_len, Ans1Enc A, AnsEnc E) {
  const int b = blockIdx.y, ck = blockIdx.x, k = threadIdx.x;
  const int count = d_len[b];
  if (count <= 32 || ck * A1_CHUNK >= count) return;
  const int64_t ci = (int64_t)b * E.C + ck;
  __shared__ u32 scan[17];
  u32 total;
  const u32 mine = A.ctxBits[ci * 256 + k];
  const u32 off = kz_wg_excl_sum(mine, scan, &total);
  u32* w = (u32*)(E.hdr + ci * E.hdrStride);
  if (k == 0) { u64 p0 = 0; a1_put(w, p0, A1_LR - 8, 3); E.hdrBits[ci] = 3 + total; }
  const u32* t = A.tab + ci * 65536 + (k << 8);
  u64 pos = 3 + (u64)off;
  u32 masks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int asz = 0, last = -1, first = -1;
  for (int s = 0; s < 256; s++) if (t[s] & 0xFFFFu) { masks[s >> 5] |= 1u << (s & 31); asz++; last = s; if (first < 0) first = s; }
  if (asz == 0) { a1_put(w, pos, 0, 1); a1_put(w, pos, 1, 1); return; }   // FULL_ALPHABET, ALPHABET_0
  if (asz == 256) { a1_put(w, pos, 0, 1); a1_put(w, pos, 0, 1); }          // FULL_ALPHABET, ALPHABET_256
  else {
    a1_put(w, pos, 1, 1);
    const int lastMask = last >> 3;
    a1_put(w, pos, (u32)lastMask, 5);
    for (int i = 0; i <= lastMask; i++) a1_put(w, pos, (masks[i >> 2] >> (8 * (i & 3))) & 0xFFu, 8);
  }
  if (asz <= 1) return;
  const int chkSize = (asz >= 64) ? 8 : 6;
  int llr = 3;
  while ((1 << llr) <= A1_LR) llr++;
  int s = first + 1;                                                        // the first symbol's frequency is implied
  for (int i = 1; i < asz; i += chkSize) {
    const int n = min(chkSize, asz - i);
    int mx = 0, got = 0, e = s;
    for (; got < n && e < 256; e++) { const u32 fq = t[e] & 0xFFFFu; if (fq) { mx = max(mx, (int)fq - 1); got++; } }
    int logMax = 0;
    while ((1 << logMax) <= mx) logMax++;
    a1_put(w, pos, (u32)logMax, llr);
    if (logMax) { got = 0; for (int j = s; got < n && j < 256; j++) { const u32 fq = t[j] & 0xFFFFu; if (fq) { a1_put(w, pos, fq - 1u, logMax); got++; } } }
    s = e;
  }
}

// encodeChunk, order 1 (:359-390): lane l is st_l, walking quarter l backwards; per step the states go st0, st1, st2, st3 into one
// buffer that fills backwards.  Step s of a chain codes symbol block[p] in context block[p - 1], p = qs + quarter - 1 - s; the
// last step codes the quarter's first byte in context 0.  The table reads do not depend on the state: the (context, symbol)
// pairs are loaded 16 steps ahead and the table entries 8 steps ahead.
__global__ __launch_bounds__(64) void k_ans1_enc(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, Ans1Enc A, AnsEnc E) {
  const int b = blockIdx.y, ck = blockIdx.x;
  const int count = d_len[b];
  const int lane = kz_lane();
  const int64_t ci = (int64_t)b * E.C + ck;
  const u8* blk = src + (int64_t)b * stride;
  u8* scr = E.scr + ci * E.scrStride;
  if (count <= 32) {                                                        // ANSRangeEncoder.java:267-270 raw
    if (ck != 0) return;
    if (lane < count) scr[lane] = blk[lane];
    if (lane == 0) { E.hdrBits[ci] = 0; E.tailOff[ci] = 0; E.tailBits[ci] = 8u * (u32)count; }
    return;
  }
  const int start = ck * A1_CHUNK;
  if (start >= count) return;
  const int len = min(count - start, A1_CHUNK);
  const u8* data = blk + start;
  __shared__ u32 recip[1 << A1_LR];                                         // Symbol.reset :488-491 by frequency
  for (int f = lane; f < (1 << A1_LR); f += 64) {
    u32 r = 0;
    if (f >= 2) { const int sh = 32 - __clz(f - 1); r = (u32)((((1ULL << (sh + 31)) + (u64)f - 1) / (u64)f) & 0xFFFFFFFFULL); }
    recip[f] = r;
  }
  __syncthreads();
  const int64_t bufLen = E.scrStride;
  const int end4 = len & -4;
  int64_t n = bufLen - 1;
  if (lane == 0) for (int i = len - 1; i >= end4; i--) scr[n - (len - 1 - i)] = data[i];
  n -= (len - end4);
  const u32* tab = A.tab + ci * 65536;
  u32 st = A1_TOP;
  int64_t idx = n;
  bool over = false;
  if (lane < 4) {
    const int quarter = end4 >> 2;
    const int qs = lane * quarter;
    // Symbol -> (xMax, bias, cmplFreq, invFreq, invShift), lr 11 (:473-496); e == 0 is a Symbol never reset: all zero
#define A1_SYMBOL(e)                                                                                                   \
    u32 fq = (e) & 0xFFFFu, cumv = (e) >> 16;                                                                          \
    if (fq >= (1u << A1_LR)) fq = (1u << A1_LR) - 1u;                                                                  \
    u32 xmax = ((A1_TOP >> A1_LR) << 16) * fq, cmpl = (fq ? (1u << A1_LR) - fq : 0u), inv, sh, bias;                   \
    if ((e) == 0u) { inv = 0; sh = 0; bias = 0; }                                                                      \
    else if (fq < 2) { inv = 0xFFFFFFFFu; sh = 32; bias = cumv + (1u << A1_LR) - 1u; }                                 \
    else { inv = recip[fq]; sh = 31 + (32 - __clz(fq - 1)); bias = cumv; }
#define A1_STEP(e)                                                                                                     \
    { A1_SYMBOL(e)                                                                                                     \
      const bool x = st >= xmax;                                                                                       \
      const uint64_t bal = kz_ballot(x) & 0xFULL;                                                                      \
      const int pre = (int)__popcll(bal & kz_lanemask_lt());                                                           \
      if (x) {                                                                                                         \
        const int64_t at = idx - 2 * pre;                                                                              \
        if (at - 1 >= A1_RESERVE) *(a1_u16_unaligned*)(scr + at - 1) = (u16)(((st & 0xFFu) << 8) | ((st >> 8) & 0xFFu)); \
        else over = true;                                                                                              \
        st >>= 16;                                                                                                     \
      }                                                                                                                \
      idx -= 2 * (int)__popcll(bal);                                                                                   \
      const u32 q = (u32)(((u64)st * (u64)inv) >> sh);                                                                 \
      st = st + bias + q * cmpl; }
    if (quarter == 0) {
      // a chunk of 1-3 bytes (the end of a block over 4 MiB): every state codes block[start - 1] in context 0 with the Symbol
      // as the latest chunk that had it left it (Symbols are reset only for present symbols, :177-186)
      const u32 x = blk[start - 1];
      u32 e = 0;
      for (int c2 = ck; c2 >= 0 && e == 0; c2--) e = A.tab[((int64_t)b * E.C + c2) * 65536 + x];
      A1_STEP(e)
    } else {
      const int steps = quarter;
      // Step s's two bytes as one load: block[p - 1] (context, low byte) and block[p] (symbol); the last step loads block[qs] and
      // codes it in context 0.  Loads and table requests are unconditional and branch-free (past the last step they read valid
      // bytes of the block's slot and are not used), and the swap into the table index happens where the entry is requested:
      // a use right after a load, or a loaded value merged across a branch, made every step wait for all its loads (vmcnt(0)).
      auto pairAt = [&](int s) -> u32 { return *(const a1_u16_unaligned*)(data + ((s < steps - 1) ? qs + quarter - 2 - s : qs)); };
      auto tabAt = [&](u32 v, int s) -> u32 { return tab[(s == steps - 1) ? (v & 0xFFu) : (((v & 0xFFu) << 8) | (v >> 8))]; };
      u32 pr[16], en[8];
#pragma unroll
      for (int j = 0; j < 16; j++) pr[j] = pairAt(j);
#pragma unroll
      for (int j = 0; j < 8; j++) { en[j] = tabAt(pr[j], j); pr[j] = pairAt(j + 16); }
      for (int s0 = 0; s0 < steps; s0 += 16) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int s = s0 + k;
          const u32 e = en[k & 7];
          en[k & 7] = tabAt(pr[(k + 8) & 15], s + 8);
          pr[(k + 8) & 15] = pairAt(s + 24);
          if (s < steps) A1_STEP(e)
        }
      }
    }
#undef A1_STEP
#undef A1_SYMBOL
  }
  idx = __shfl(idx, 0, 64);
  over = kz_ballot(over) != 0;
  n = idx + 1;
  const u32 payload = (u32)(bufLen - n);
  u32 vlen = 1; { u32 v = payload; while (v >= 128) { v >>= 7; vlen++; } }
  const int64_t tail = n - 16 - (int64_t)vlen;
  if (over) {                             // (the reference's buffer would have overflowed too): more bits than the block's raw copy
    if (lane == 0) { E.tailOff[ci] = 0; E.tailBits[ci] = (u32)(8 * bufLen); }
    return;
  }
  if (lane == 0) {
    u32 v = payload; int64_t p = tail;
    while (v >= 128) { scr[p++] = (u8)(0x80 | (v & 0x7F)); v >>= 7; }     // EntropyUtils.java:259-276
    scr[p++] = (u8)v;
    E.tailOff[ci] = (u32)tail; E.tailBits[ci] = 8u * (payload + 16 + vlen);
  }
  if (lane < 4) {
    u8* p = scr + tail + vlen + 4 * lane;
    p[0] = (u8)(st >> 24); p[1] = (u8)(st >> 16); p[2] = (u8)(st >> 8); p[3] = (u8)st;
  }
}

static int a1_max_len(const kz_batch& bt) { int m = 0; for (int b = 0; b < bt.B; b++) m = std::max(m, bt.h_len[b]); return m; }
static int64_t a1_scr_stride(int maxN) { const int64_t cl = std::min(maxN, A1_CHUNK); return (int64_t)kz_align((size_t)(cl + (cl >> 3) + 65536), 256); }

size_t kz_ans1_scratch(int B, int maxN, bool decode) {
  const size_t C = (size_t)std::max(1, (maxN + A1_CHUNK - 1) / A1_CHUNK);   // what the stages allocate per block
  if (decode) return (size_t)B * C * (256 * 8 + 256 * 4 + 65536 * 4 + 256 * 2048 * 4 + 64 + 256 * 6) + (size_t)B * 64 + 65536;
  return (size_t)B * C * (65536 * 4 + 256 * 4 + A1_HDR_BYTES + (size_t)a1_scr_stride(maxN) + 64) + (size_t)B * 64 + 65536;
}

int kz_stage_ans1_encode(kz_ctx* ctx, kz_batch& bt, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits) {
  const int B = bt.B;
  const int maxN = a1_max_len(bt);
  const int chunks = (maxN + A1_CHUNK - 1) / A1_CHUNK;
  AnsEnc E; Ans1Enc A;
  E.C = std::max(chunks, 1);
  E.chunk = A1_CHUNK; E.hdrStride = A1_HDR_BYTES; E.scrStride = a1_scr_stride(std::max(maxN, 1)); E.outCap = outStride;
  const size_t NC = (size_t)B * E.C;
  E.hdr = (u8*)kz_arena_alloc(ctx, NC * A1_HDR_BYTES);
  E.scr = (u8*)kz_arena_alloc(ctx, NC * (size_t)E.scrStride);
  E.hdrBits = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.tailOff = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.tailBits = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.bitOff = (u64*)kz_arena_alloc(ctx, NC * 8);
  A.tab = (u32*)kz_arena_alloc(ctx, NC * 65536 * 4);
  A.ctxBits = (u32*)kz_arena_alloc(ctx, NC * 256 * 4);
  if (!E.hdr || !E.scr || !E.bitOff || !A.tab || !A.ctxBits) { snprintf(ctx->err, sizeof(ctx->err), "ans1 encode: arena overflow"); return -KZ_ERR_DEVICE; }
  hipStream_t st = ctx->stream;
  KZ_HIP(hipMemsetAsync(E.hdrBits, 0, NC * 4, st));
  KZ_HIP(hipMemsetAsync(E.tailBits, 0, NC * 4, st));
  if (chunks > 0) {
    KZ_HIP(hipMemsetAsync(E.hdr, 0, NC * A1_HDR_BYTES, st));
    KZ_HIP(hipMemsetAsync(A.tab, 0, NC * 65536 * 4, st));
    const int segs = (std::min(maxN, A1_CHUNK) + A1_SEG - 1) / A1_SEG;
    KZ_LAUNCH(ctx, KID_ANS1_HIST, k_ans1_hist, dim3(segs * 4, chunks, B), dim3(KZ_WG), bt.buf[bt.cur], bt.stride, bt.d_len, A, E.C);
    KZ_LAUNCH(ctx, KID_ANS1_NORM, k_ans1_norm, dim3(256, chunks, B), dim3(64), bt.d_len, A, E.C);
    KZ_LAUNCH(ctx, KID_ANS1_HDR, k_ans1_hdr, dim3(chunks, B), dim3(256), bt.d_len, A, E);
    KZ_LAUNCH(ctx, KID_ANS1_ENC, k_ans1_enc, dim3(chunks, B), dim3(64), bt.buf[bt.cur], bt.stride, bt.d_len, A, E);
  }
  return kz_chunk_enc_finish(ctx, bt, E, chunks, out, outStride, d_hdrBytes, d_bits, 32);
}

// =================================================================================================
// decode.  Events are keyed chunk * 4 + kind so that the lowest chunk's wins (the reference stops at the first), as in kz_ans.hip.
#define A1_EV_NONE 0x7FFFFFFF
#define A1_EV_FAIL 0
#define A1_EV_SKIP 1
#define A1_EV_STOP 2
struct Ans1Dec {
  u64* ctxBit;       // [B][C][256] bit position of each context header
  int32_t* asz;      // [B][C][256] alphabet size of each context (0: the context keeps its tables from an earlier chunk)
  u32* rec;          // [B][C][256][256] {Symbol.freq | cumulative frequency << 16} of the contexts with asz > 0
  u32* fast;         // [B][C][256][2048] {sym | freq << 8 | (slot - cum) << 20} for chunks with lr <= 11; 0: take the slow path
  u64* payBit;       // [B][C] bit position of the chunk's varint
  int32_t* lr;       // [B][C]
  int32_t* event;    // [B]
  int32_t* nIdx;     // [B] chunks to decode
  u64* endBit;       // [B][C] bit position behind each chunk's payload (where the reference stops reading after a chunk that stops early)
  int C;
};

__device__ __forceinline__ u32 a1_peek(const u8* __restrict__ p, u64 pos, int count) {   // count <= 25
  const u64 by = pos >> 3;
  u32 acc = ((u32)p[by] << 24) | ((u32)p[by + 1] << 16) | ((u32)p[by + 2] << 8) | (u32)p[by + 3];
  acc <<= (pos & 7);
  return count ? (acc >> (32 - count)) : 0;
}

// one lane per block: decodeHeader (:452-544) of every chunk -- with its exceptions -- and the chunk sizes (:357-380)
__global__ void k_ans1_dec_index(const u8* __restrict__ in, int64_t inStride, const int64_t* __restrict__ d_bitOff,
                                 const int64_t* __restrict__ d_bitEnd, const int32_t* __restrict__ d_len, Ans1Dec D, int B, long long* __restrict__ endOut) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int count = d_len[b];
  const u8* p = in + (int64_t)b * inStride;
  u64 pos = (u64)d_bitOff[b];
  const u64 endBits = (u64)d_bitEnd[b];
  int event = A1_EV_NONE, nIdx = 0;
  u32 bufLen = 0;
#define A1_NEED(nb) if (pos + (u64)(nb) > endBits) { event = c * 4 + A1_EV_FAIL; goto done; }
  if (count > 32) {
    const int chunks = (count + A1_CHUNK - 1) / A1_CHUNK;
    for (int c = 0; c < chunks; c++) {
      const int64_t ci = (int64_t)b * D.C + c;
      A1_NEED(3)
      const int lr = 8 + (int)a1_peek(p, pos, 3); pos += 3;
      const int scale = 1 << lr;
      D.lr[ci] = lr;
      int llr = 3;
      while ((1 << llr) <= lr) llr++;
      int totalAlpha = 0;
      for (int k = 0; k < 256; k++) {
        D.ctxBit[ci * 256 + k] = pos;
        int asz = 0;
        A1_NEED(2)
        if (a1_peek(p, pos, 1) == 0) { asz = (a1_peek(p, pos + 1, 1) == 1) ? 0 : 256; pos += 2; }
        else {
          A1_NEED(6)
          const int lastMask = (int)a1_peek(p, pos + 1, 5); pos += 6;
          A1_NEED(8 * (lastMask + 1))
          for (int i = 0; i <= lastMask; i++) { asz += __popc(a1_peek(p, pos, 8)); pos += 8; }
        }
        D.asz[ci * 256 + k] = asz;
        if (asz == 0) continue;
        const int chkSize = (asz >= 64) ? 8 : 6;
        int sum = 0;
        for (int i = 1; i < asz; i += chkSize) {
          A1_NEED(llr)
          const int logMax = (int)a1_peek(p, pos, llr); pos += llr;
          if ((1 << logMax) > scale) { event = c * 4 + A1_EV_FAIL; goto done; }
          const int endj = min(i + chkSize, asz);
          if (logMax == 0) { sum += endj - i; continue; }
          A1_NEED(logMax * (endj - i))
          for (int j = i; j < endj; j++) {
            const int fq = 1 + (int)a1_peek(p, pos, logMax); pos += logMax;
            if (fq >= scale) { event = c * 4 + A1_EV_FAIL; goto done; }
            sum += fq;
          }
        }
        if (scale <= sum) { event = c * 4 + A1_EV_FAIL; goto done; }
        totalAlpha += asz;
      }
      if (totalAlpha == 0) { event = c * 4 + A1_EV_FAIL; goto done; }        // :213-215: decode returns startChunk != count
      D.payBit[ci] = pos;
      // varint (EntropyUtils.java:284-300)
      A1_NEED(8)
      u32 v = a1_peek(p, pos, 8); pos += 8;
      u32 sz = v & 0x7F; int shift = 7;
      while (v >= 128) { A1_NEED(8) v = a1_peek(p, pos, 8); pos += 8; sz |= (v & 0x7F) << shift; if (shift == 28) break; shift += 7; }
      if ((int)sz >= (int)A1_MAX_CHUNK_SIZE) { event = c * 4 + A1_EV_SKIP; goto done; }   // :360-361 (a negative int passes)
      A1_NEED(128)
      pos += 128;
      const u32 clen = (u32)min(count - c * A1_CHUNK, A1_CHUNK);
      bufLen = max(bufLen, max(2u * clen, 256u));                           // this.buffer only grows (:369-374)
      if (sz > bufLen) { event = c * 4 + A1_EV_FAIL; goto done; }          // readBits past the array end (or a negative size) throws
      A1_NEED(8ULL * sz)
      pos += 8ULL * sz;
      D.endBit[ci] = pos;
      nIdx = c + 1;
    }
  } else {                                                                  // :193-196
    pos += 8ULL * (u64)(count > 0 ? count : 0);
    if (pos > endBits) event = A1_EV_FAIL;
  }
done:
#undef A1_NEED
  if (endOut) endOut[b] = (long long)pos;
  D.event[b] = event;
  D.nIdx[b] = nIdx;
}

// one wave per (chunk, context) with asz > 0: the frequencies (validated by the index pass), the Symbol records and the slot table
__global__ __launch_bounds__(64) void k_ans1_dec_table(const u8* __restrict__ in, int64_t inStride, const int32_t* __restrict__ d_len, Ans1Dec D) {
  const int b = blockIdx.z, ck = blockIdx.y, k = blockIdx.x;
  const int count = d_len[b];
  if (count <= 32 || ck >= D.nIdx[b]) return;
  const int lane = kz_lane();
  const int64_t ci = (int64_t)b * D.C + ck;
  const int64_t cx = ci * 256 + k;
  const int lr = D.lr[ci];
  const int scale = 1 << lr;
  const int asz = D.asz[cx];
  u32* fast = D.fast + cx * 2048;
  if (asz == 0) {
    if (lr <= A1_FAST_LR) for (int x = lane; x < scale; x += 64) fast[x] = 0;
    return;
  }
  __shared__ u32 freq[256];
  __shared__ u16 cumf[256];
  __shared__ u8 alpha[256];
  for (int i = lane; i < 256; i += 64) freq[i] = 0;
  __syncthreads();
  if (lane == 0) {
    const u8* p = in + (int64_t)b * inStride;
    u64 pos = D.ctxBit[cx];
    int n = 0;
    if (a1_peek(p, pos, 1) == 0) { for (int i = 0; i < 256; i++) alpha[i] = (u8)i; n = 256; pos += 2; }
    else {
      const int lastMask = (int)a1_peek(p, pos + 1, 5); pos += 6;
      for (int i = 0; i <= lastMask; i++) {
        const u32 m = a1_peek(p, pos, 8); pos += 8;
        for (int j = 0; j < 8; j++) if (m & (1u << j)) alpha[n++] = (u8)((i << 3) + j);
      }
    }
    int llr = 3;
    while ((1 << llr) <= lr) llr++;
    const int chkSize = (n >= 64) ? 8 : 6;
    int sum = 0;
    for (int i = 1; i < n; i += chkSize) {
      const int logMax = (int)a1_peek(p, pos, llr); pos += llr;
      const int endj = min(i + chkSize, n);
      for (int j = i; j < endj; j++) {
        const int fq = (logMax == 0) ? 1 : 1 + (int)a1_peek(p, pos, logMax);
        pos += logMax;
        freq[alpha[j]] = (u32)fq; sum += fq;
      }
    }
    freq[alpha[0]] = (u32)(scale - sum);
  }
  __syncthreads();
  u32 cum = 0;
  u32* rec = D.rec + cx * 256;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const u32 fv = freq[q * 64 + lane];
    const u32 inc = kz_wave_incl_sum(fv);
    const u32 c0 = cum + inc - fv;
    cum += __shfl(inc, 63, 64);
    cumf[q * 64 + lane] = (u16)c0;
    const u32 fc = fv >= (u32)scale ? (u32)scale - 1u : fv;                  // Symbol.reset :576-579
    rec[q * 64 + lane] = fc | (c0 << 16);
  }
  __syncthreads();
  if (lr > A1_FAST_LR) return;
  // slot x: the last symbol whose cumulative frequency is <= x (symbols of frequency 0 share their successor's value)
  const int per = scale >> 6;                                               // scale >= 256: 4 .. 32 slots per lane
  const int x0 = lane * per;
  int lo = 0, hi = 256;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int)cumf[mid] <= x0) lo = mid; else hi = mid; }
  int sy = lo;
  int nextAt = (sy + 1 < 256) ? (int)cumf[sy + 1] : 0x7FFFFFFF;
  for (int x = x0; x < x0 + per; x++) {
    while (sy < 255 && (nextAt <= x || freq[sy] == 0)) { sy++; nextAt = (sy + 1 < 256) ? (int)cumf[sy + 1] : 0x7FFFFFFF; }
    const u32 fc = freq[sy] >= (u32)scale ? (u32)scale - 1u : freq[sy];
    fast[x] = (u32)sy | (fc << 8) | ((u32)(x - cumf[sy]) << 20);
  }
}

// The reference's tables for context k at chunk ck where this chunk's own table does not answer (the context is empty in this chunk
// and keeps its tables from an earlier one, or lr > 11).  f2s[k] is an array as long as the largest scale it was ever filled at,
// entry x written by the latest chunk whose scale exceeds x; symbols[k][s] is the Symbol of the latest chunk in which s was present.
// Returns false where the Java indexes past the array (a context never filled: new byte[0], :142).
__device__ bool a1_slow(const Ans1Dec& D, int b, int ck, int k, u32 x, u32& sym, u32& fq, u32& cum) {
  int c2 = ck;
  for (; c2 >= 0; c2--) { const int64_t ci = (int64_t)b * D.C + c2; if (D.asz[ci * 256 + k] > 0 && (1u << D.lr[ci]) > x) break; }
  if (c2 < 0) return false;
  const u32* r2 = D.rec + (((int64_t)b * D.C + c2) * 256 + k) * 256;
  int lo = 0, hi = 256;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((r2[mid] >> 16) <= x) lo = mid; else hi = mid; }
  while (lo > 0 && (r2[lo] & 0xFFFFu) == 0) lo--;                                     // ties: the present symbol is the first of its run
  sym = (u32)lo;
  for (int c3 = ck; c3 >= c2; c3--) {
    const int64_t cx = ((int64_t)b * D.C + c3) * 256 + k;
    if (D.asz[cx] > 0) { const u32 r = D.rec[cx * 256 + sym]; if (r & 0xFFFFu) { fq = r & 0xFFFFu; cum = r >> 16; return true; } }
  }
  return false;                                                             // (not reached: chunk c2 has the symbol)
}

// decodeChunkV2 order 1 (:406-432): lane j is st(3 - j), quarter 3 - j; per step lanes 0..3 = st3, st2, st1, st0 take their bytes
// from one cursor.  The context restarts at 0 in every quarter.
__global__ __launch_bounds__(64) void k_ans1_dec_chunk(const u8* __restrict__ in, int64_t inStride, const int64_t* __restrict__ d_bitOff,
                                                        const int32_t* __restrict__ d_len, Ans1Dec D, u8* __restrict__ dst, int64_t stride) {
  const int b = blockIdx.y, ck = blockIdx.x;
  const int count = d_len[b];
  const int lane = kz_lane();
  const u8* p = in + (int64_t)b * inStride;
  u8* o = dst + (int64_t)b * stride;
  if (count <= 32) {
    if (ck != 0) return;
    if (lane < count) o[lane] = (u8)a1_peek(p, (u64)d_bitOff[b] + 8ULL * lane, 8);
    return;
  }
  const int start = ck * A1_CHUNK;
  if (start >= count || ck >= D.nIdx[b]) return;
  const int len = min(count - start, A1_CHUNK);
  const int64_t ci = (int64_t)b * D.C + ck;
  const int lr = D.lr[ci];
  const u32 mask = (1u << lr) - 1u;
  const bool fastOk = lr <= A1_FAST_LR;
  u64 pos = D.payBit[ci];
  u32 v = a1_peek(p, pos, 8); pos += 8;
  u32 sz = v & 0x7F; int shift = 7;
  while (v >= 128) { v = a1_peek(p, pos, 8); pos += 8; sz |= (v & 0x7F) << shift; if (shift == 28) break; shift += 7; }
  u32 st = 0;
  if (lane < 4) { const u64 sp = pos + 32ULL * (3 - lane); st = (a1_peek(p, sp, 16) << 16) | a1_peek(p, sp + 16, 16); }
  pos += 128;
  const u64 payBit = pos, payByte = pos >> 3;
  const u32 payShift = (u32)(pos & 7);
  const bool winOk = payByte + (u64)sz + 24 <= (u64)inStride;              // 16-byte reads at the cursor stay inside the block's slot
  const int end4 = len & -4;
  const int quarter = end4 >> 2;
  u32 n = 0;
  bool fail = false;
  if (lane < 4) {
    const int q = 3 - lane;
    u8* oq = o + start + q * quarter;
    u32 prv = 0;
    const u32* fastBase = D.fast + ci * 256 * 2048;
    for (int s = 0; s < quarter; s++) {
      // the next 8 payload bytes, requested before the table read they do not depend on
      u64 win = 0;
      if (winOk) {                                                          // (past sz every byte reads as 0: the address stops there)
        const u32 nn = n < sz ? n : sz;
        const u64 hiw = __builtin_bswap64(*(const a1_u64_unaligned*)(p + payByte + nn));
        const u64 low = __builtin_bswap64(*(const a1_u64_unaligned*)(p + payByte + nn + 8));
        win = payShift ? ((hiw << payShift) | (low >> (64 - payShift))) : hiw;
      }
      const u32 x = st & mask;
      u32 e = fastOk ? fastBase[(prv << 11) + x] : 0u;
      u32 cur;
      if (e != 0) {
        cur = e & 0xFFu;
        st = ((e >> 8) & 0xFFFu) * (st >> lr) + (e >> 20);
      } else {
        u32 fq = 0, cm = 0;
        if (!a1_slow(D, b, ck, (int)prv, x, cur, fq, cm)) { fail = true; cur = 0; }
        st = fq * (st >> lr) + x - cm;
      }
      if (kz_ballot(fail) & 0xFULL) break;
      oq[s] = (u8)cur;
      const bool need = (int)st < (int)A1_TOP;
      const uint64_t bal = kz_ballot(need) & 0xFULL;
      if (need) {
        const u32 off = 2u * (u32)__popcll(bal & kz_lanemask_lt());
        const u32 at = n + off;
        u32 hi, lo;
        if (winOk) { hi = (u32)(win >> (56 - 8 * off)) & 0xFFu; lo = (u32)(win >> (48 - 8 * off)) & 0xFFu; }
        else { hi = (at < sz) ? a1_peek(p, payBit + 8ULL * at, 8) : 0u; lo = (at + 1 < sz) ? a1_peek(p, payBit + 8ULL * (at + 1), 8) : 0u; }
        if (winOk) { hi = (at < sz) ? hi : 0u; lo = (at + 1 < sz) ? lo : 0u; }
        st = (st << 16) | (hi << 8) | lo;
      }
      n += 2u * (u32)__popcll(bal);
      prv = cur;
    }
  }
  if (kz_ballot(fail)) { if (lane == 0) atomicMin(&D.event[b], ck * 4 + A1_EV_FAIL); return; }
  n = __shfl(n, 0, 64);
  if (lane < len - end4) { const u32 at = n + (u32)lane; o[start + end4 + lane] = (at < sz) ? (u8)a1_peek(p, payBit + 8ULL * at, 8) : 0; }
  n += (u32)(len - end4);
  if (lane == 0 && n != sz) atomicMin(&D.event[b], ck * 4 + A1_EV_STOP);   // :439
}

__global__ __launch_bounds__(64) void k_ans1_dec_fin(const int32_t* __restrict__ d_len, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                      Ans1Dec D, u8* __restrict__ dst, int64_t stride, long long* __restrict__ endOut) {
  const int b = blockIdx.x, lane = kz_lane();
  const int count = d_len[b];
  const int ev = D.event[b];
  if (lane == 0) { d_len2[b] = count; d_flag[b] = (ev == A1_EV_NONE || (ev & 3) != A1_EV_FAIL) ? 1 : 0; }
  if (ev == A1_EV_NONE || (ev & 3) == A1_EV_FAIL) return;
  // the index pass walked the chunks behind a chunk that stops early; the reference stops reading behind its payload
  if (lane == 0 && endOut && (ev & 3) == A1_EV_STOP) endOut[b] = (long long)D.endBit[(int64_t)b * D.C + (ev >> 2)];
  const int64_t from = (int64_t)((ev >> 2) + ((ev & 3) == A1_EV_STOP ? 1 : 0)) * A1_CHUNK;
  u8* o = dst + (int64_t)b * stride;
  for (int64_t i = from + lane; i < count; i += 64) o[i] = 0;
}

int kz_stage_ans1_decode(kz_ctx* ctx, kz_batch& bt, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd) {
  const int B = bt.B;
  const int maxN = a1_max_len(bt);
  const int chunks = maxN > 32 ? (maxN + A1_CHUNK - 1) / A1_CHUNK : (maxN > 0 ? 1 : 0);
  Ans1Dec D;
  D.C = std::max(chunks, 1);
  const size_t NC = (size_t)B * D.C;
  D.ctxBit = (u64*)kz_arena_alloc(ctx, NC * 256 * 8);
  D.asz = (int32_t*)kz_arena_alloc(ctx, NC * 256 * 4);
  D.rec = (u32*)kz_arena_alloc(ctx, NC * 65536 * 4);
  D.fast = (u32*)kz_arena_alloc(ctx, NC * 256 * 2048 * 4);
  D.payBit = (u64*)kz_arena_alloc(ctx, NC * 8);
  D.lr = (int32_t*)kz_arena_alloc(ctx, NC * 4);
  D.event = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  D.nIdx = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  D.endBit = (u64*)kz_arena_alloc(ctx, NC * 8);
  if (!D.ctxBit || !D.asz || !D.rec || !D.fast || !D.payBit || !D.lr || !D.event || !D.nIdx || !D.endBit) { snprintf(ctx->err, sizeof(ctx->err), "ans1 decode: arena overflow"); return -KZ_ERR_DEVICE; }
  u8* dst = bt.buf[bt.cur ^ 1];
  KZ_LAUNCH(ctx, KID_ANS1_DEC_INDEX, k_ans1_dec_index, dim3((B + 63) / 64), dim3(64), in, inStride, d_bitOff, d_bitEnd, bt.d_len, D, B, ctx->d_endBits);
  if (chunks > 0) {
    if (maxN > 32) KZ_LAUNCH(ctx, KID_ANS1_DEC_TABLE, k_ans1_dec_table, dim3(256, chunks, B), dim3(64), in, inStride, bt.d_len, D);
    KZ_LAUNCH(ctx, KID_ANS1_DEC_CHUNK, k_ans1_dec_chunk, dim3(chunks, B), dim3(64), in, inStride, d_bitOff, bt.d_len, D, dst, bt.stride);
  }
  KZ_LAUNCH(ctx, KID_ANS1_DEC_FIN, k_ans1_dec_fin, dim3(B), dim3(64), bt.d_len, bt.d_len2, bt.d_flag, D, dst, bt.stride, ctx->d_endBits);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
