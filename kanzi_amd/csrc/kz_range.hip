// kz_range.hip -- order-0 range coder (entropy id 4, RANGE) for gfx950.
//
// Replaces K/entropy/RangeEncoder.java:244-282 (encode), :328-331 (rebuildStatistics), :159-175 (updateFrequencies), :186-228
// (encodeHeader), :292-316 (encodeByte) and K/entropy/RangeDecoder.java:254-292 (decode), :161-239 (decodeHeader), :300-327
// (decodeByte); K/entropy/EntropyUtils.java:141-250 (normalizeFrequencies, kz_normalize.h), :38-75 (encodeAlphabet).
// EntropyCodecFactory builds both with the defaults: 32 KiB chunks, logRange 12 (RangeEncoder.java:65-70).
//
// Encode: the statistics reset every 32 KiB chunk and the low / range registers with them, so a block is up to 128 independent
// chains: one wave64 per chunk.  The wave builds the histogram (LDS, ballot-aggregated), normalises it (kz_normalize.h) and writes the
// header; the chain itself is wave-uniform (every lane computes the same low / range, so it costs one lane's instructions), the
// lanes feed it: each row of 256 input bytes is loaded as one dword per lane and translated to {cumFreq, freq} records through the
// LDS table by all lanes at once, the chain takes them with v_readlane; the 28-bit groups are packed into 32-bit words that lane
// (n & 63) holds, and 64 words leave with one 256-byte store.  The chunks' bit strings are joined by kz_ans.hip's scan + concat.
//
// Decode: nothing in the stream says where a chunk ends, so a block is ONE chain (as FPAQ's): one wave per block.  Per chunk the wave
// parses and validates the header, scans the frequencies and fills the f2s table in LDS by slot; then the chain runs wave-uniform,
// one signed 64-bit division per byte (rg_quot), the decoded bytes collected one per lane and stored 64 at a time.
//
// Loops that depend on the stream or the coder state are bounded: the normalisation loop by RG_MAX_PASSES per byte,
// the header parse by the alphabet (<= 256 symbols), everything else by the block's length.
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_chunk.h"
#include "kz_normalize.h"
#include <algorithm>

typedef uint16_t u16;

#define RG_TOP 0x0FFFFFFFFFFFFFFFULL        // RangeEncoder.java:50
#define RG_BOTTOM 0x000000000000FFFFULL     // :55
#define RG_MASK 0x0FFFFFFF00000000ULL       // :60
#define RG_CHUNK 32768                      // :65
#define RG_LR 12                            // :70
#define RG_HDR_BYTES 512                    // longest header: 262 alphabet bits + 3 + 43 groups x (4 + 6 x 12) < 3 600 bits
// Per-chunk payload buffer.  With L = log2(range): a byte lowers L by log2(scale / freq) <= lr (freq >= 1) plus the floor of
// range >> lr (range >= 2^16, lr <= 12: below log2(17/16) < 0.09 bit); every 28-bit group raises it by 28; a low-range event
// (range = -low & 0xFFFF) lowers it by at most 16; L starts at 60 and stays below 60.  So the groups hold fewer than
// n (lr + 0.09) + 16 K bits for n bytes and K low-range events, and the flush adds 60: for n = 32 768, lr = 12 that is
// 396 225 + 16 K bits.  50 KiB = 409 600 bits leave room for K = 836 events; a chunk of random bytes has about one (it needs low within
// 2^16 of a multiple of 2^32 while range <= 2^16).  The cursor is checked all the same: a chunk that does not fit fails its block.
#define RG_SCRATCH 51200
// A byte whose normalisation loop makes more passes than this never leaves it (range == 0): a non-zero range survives at most
// three shifts by 28 bits, and from the second pass on low's 28 low bits are zero, so the low-range branch gives range = 0 too.
// tests/rangemodel.py has the same bound and the argument why valid input stays below it.
#define RG_MAX_PASSES 8

typedef u64 __attribute__((aligned(1))) rg_u64_unaligned;

// ---- single-lane MSB-first bit writer into a zeroed buffer (DefaultOutputBitStream.java:103-123) ----
struct RgBitW { u8* p; u32 pos; };
__device__ __forceinline__ void rg_put(RgBitW& w, u32 v, int count) {
  while (count > 0) {
    const int bitoff = w.pos & 7, room = 8 - bitoff;
    const int take = count < room ? count : room;
    const u32 bits = (v >> (count - take)) & ((1u << take) - 1u);
    w.p[w.pos >> 3] |= (u8)(bits << (room - take));
    w.pos += take; count -= take;
  }
}

// ---- the chain's output: 32-bit words, big endian, lane (n & 63) holds word n until 64 of them leave with one store ----
struct RgOut { u32* w; u32 cap; u32 n; u32 hold; u64 acc; int na; bool over; };
__device__ __forceinline__ void rg_word(RgOut& o, u32 word, int lane) {
  o.hold = (lane == (int)(o.n & 63u)) ? __builtin_bswap32(word) : o.hold;
  o.n++;
  if ((o.n & 63u) == 0) {                                         // cap is a multiple of 64 words: a row is inside or outside as a whole
    if (o.n <= o.cap) o.w[o.n - 64 + lane] = o.hold; else o.over = true;
  }
}
__device__ __forceinline__ void rg_emit(RgOut& o, u32 v, int bits, int lane) {    // bits <= 32, v < 2^bits
  o.acc = (o.acc << bits) | (u64)v;
  o.na += bits;
  if (o.na >= 32) { o.na -= 32; rg_word(o, (u32)(o.acc >> o.na), lane); }
}

// =================================================================================================
// encode: one wave per chunk
__global__ __launch_bounds__(64) void k_range_enc_chunk(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len,
                                                         AnsEnc E, int32_t* __restrict__ fail) {
  const int b = blockIdx.y, ck = blockIdx.x;
  const int count = d_len[b];
  const int start = ck * RG_CHUNK;
  if (start >= count) return;
  const int lane = kz_lane();
  const int64_t ci = (int64_t)b * E.C + ck;
  const u8* blk = src + (int64_t)b * stride;
  const int len = min(count - start, RG_CHUNK);

  __shared__ u32 hist[256];
  __shared__ u16 nfreq[256];
  __shared__ u8 alpha[256];
  __shared__ u32 symTab[256];                                   // cumFreq | freq << 16
  __shared__ u32 hbuf[RG_HDR_BYTES / 4];

  for (int i = lane; i < 256; i += 64) hist[i] = 0;
  for (int i = lane; i < RG_HDR_BYTES / 4; i += 64) hbuf[i] = 0;
  __syncthreads();
  // ---- Global.computeHistogramOrder0 (K/Global.java:274-322) ----
  for (int i = lane * 4; i < len; i += 256) {
    u32 w = 0; const int nb = min(4, len - i);
    if (nb == 4 && ((start + i) & 3) == 0) w = *(const u32*)(blk + start + i);
    else for (int k = 0; k < nb; k++) w |= (u32)blk[start + i + k] << (8 * k);
    for (int k = 0; k < 4; k++) {
      const bool valid = k < nb;
      const u32 c = (w >> (8 * k)) & 0xFF;
      const uint64_t peers = kz_match8(c, valid);
      if (valid && (peers & kz_lanemask_lt()) == 0) atomicAdd(&hist[c], (u32)__popcll(peers));
    }
  }
  __syncthreads();
  int lr = RG_LR;                                                 // RangeEncoder.java:259-263
  while (lr > 8 && (1 << lr) > len) lr--;
  const u32 scale = 1u << lr;
  u32 f[4];
#pragma unroll
  for (int q = 0; q < 4; q++) f[q] = hist[q * 64 + lane];
  const u32 alphabetSize = kz_normalize_wave(f, (u32)len, scale);
  // ---- cumFreqs (:166-170), alphabet ----
  u32 cum = 0, apos = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const u32 inc = kz_wave_incl_sum(f[q]);
    const int s = q * 64 + lane;
    symTab[s] = (cum + inc - f[q]) | (f[q] << 16);
    nfreq[s] = (u16)f[q];
    cum += __shfl(inc, 63, 64);
    const uint64_t bal = kz_ballot(f[q] != 0);
    if (f[q] != 0) alpha[apos + (u32)__popcll(bal & kz_lanemask_lt())] = (u8)s;
    apos += (u32)__popcll(bal);
  }
  __syncthreads();
  // ---- encodeHeader :186-228, lane 0 ----
  if (lane == 0) {
    RgBitW w{(u8*)hbuf, 0};
    if (alphabetSize == 256) { rg_put(w, 0, 1); rg_put(w, 0, 1); }          // FULL_ALPHABET, ALPHABET_256
    else {
      rg_put(w, 1, 1);
      const int lastMask = alpha[alphabetSize - 1] >> 3;
      rg_put(w, (u32)lastMask, 5);
      for (int i = 0; i <= lastMask; i++) {
        u32 m = 0;
        for (int j = 0; j < 8; j++) if (nfreq[i * 8 + j] != 0) m |= 1u << j;
        rg_put(w, m, 8);
      }
    }
    rg_put(w, (u32)(lr - 8), 3);
    const int chkSize = (alphabetSize >= 64) ? 8 : 6;
    int llr = 3;
    while ((1 << llr) <= lr) llr++;
    for (int i = 1; i < (int)alphabetSize; i += chkSize) {
      const int endj = (i + chkSize < (int)alphabetSize) ? i + chkSize : (int)alphabetSize;
      int mx = (int)nfreq[alpha[i]] - 1;
      for (int j = i + 1; j < endj; j++) { const int v = (int)nfreq[alpha[j]] - 1; if (v > mx) mx = v; }
      int logMax = 0;
      while ((1 << logMax) <= mx) logMax++;
      rg_put(w, (u32)logMax, llr);
      if (logMax == 0) continue;
      for (int j = i; j < endj; j++) rg_put(w, (u32)nfreq[alpha[j]] - 1u, logMax);
    }
    E.hdrBits[ci] = w.pos;
    E.tailOff[ci] = 0;
  }
  __syncthreads();
  { u32* hdr = (u32*)(E.hdr + ci * E.hdrStride); for (int i = lane; i < RG_HDR_BYTES / 4; i += 64) hdr[i] = hbuf[i]; }
  if (alphabetSize <= 1) {                                        // :265-269 header only, no flush
    if (lane == 0) E.tailBits[ci] = 0;
    return;
  }
  // ---- encodeByte :292-316 for every byte, wave-uniform ----
  RgOut o{(u32*)(E.scr + ci * E.scrStride), (u32)(E.scrStride >> 2), 0u, 0u, 0ULL, 0, false};
  u64 low = 0, range = RG_TOP;
  bool stuck = false;
  u32 wNext = 0;
  { const int i = lane * 4; if (i < len) { if (i + 4 <= len) wNext = *(const u32*)(blk + start + i); else for (int k = 0; k < len - i; k++) wNext |= (u32)blk[start + i + k] << (8 * k); } }
  for (int row = 0; row < len && !stuck; row += 256) {
    const u32 w = wNext;
    { const int i = row + 256 + lane * 4; wNext = 0;             // the next row is requested a row ahead (chunks start 4-byte aligned)
      if (i < len) { if (i + 4 <= len) wNext = *(const u32*)(blk + start + i); else for (int k = 0; k < len - i; k++) wNext |= (u32)blk[start + i + k] << (8 * k); } }
    const int e0 = (int)symTab[w & 0xFF], e1 = (int)symTab[(w >> 8) & 0xFF], e2 = (int)symTab[(w >> 16) & 0xFF], e3 = (int)symTab[w >> 24];
    const int rowCnt = min(256, len - row);
    for (int j = 0; j < rowCnt && !stuck; j += 4) {
      const int jl = j >> 2;
      const u32 ent[4] = {(u32)__builtin_amdgcn_readlane(e0, jl), (u32)__builtin_amdgcn_readlane(e1, jl),
                          (u32)__builtin_amdgcn_readlane(e2, jl), (u32)__builtin_amdgcn_readlane(e3, jl)};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (j + k >= rowCnt || stuck) break;
        const u64 cumFreq = ent[k] & 0xFFFFu, freq = ent[k] >> 16;
        range >>= lr;
        low += cumFreq * range;
        range *= freq;
        for (int pass = 0;; pass++) {
          if (((low ^ (low + range)) & RG_MASK) != 0) {
            if ((int64_t)range > (int64_t)RG_BOTTOM) break;
            range = (0ULL - low) & RG_BOTTOM;
          }
          if (pass >= RG_MAX_PASSES) { stuck = true; break; }
          rg_emit(o, (u32)(low >> 32) & 0x0FFFFFFFu, 28, lane);
          range <<= 28;
          low <<= 28;
        }
      }
    }
  }
  rg_emit(o, (u32)(low >> 28), 32, lane);                        // writeBits(low, 60) :277
  rg_emit(o, (u32)low & 0x0FFFFFFFu, 28, lane);
  const u32 bits = 32u * o.n + (u32)o.na;
  if (o.na > 0) rg_word(o, (u32)(o.acc << (32 - o.na)), lane);
  if ((o.n & 63u) != 0) {
    const u32 idx = (o.n & ~63u) + (u32)lane;
    if (o.n > o.cap) o.over = true;
    else if ((u32)lane < (o.n & 63u)) o.w[idx] = o.hold;
  }
  if (lane == 0) {
    const bool bad = o.over || stuck;
    E.tailBits[ci] = bad ? 0u : bits;
    if (bad) { E.hdrBits[ci] = 0; atomicOr(&fail[b], 1); }
  }
}

// per block: a chunk that did not fit its buffer (or whose chain never ended) fails the block: no bits, flag 0
__global__ void k_range_enc_fin(const int32_t* __restrict__ fail, int64_t* __restrict__ d_bits, int32_t* __restrict__ d_flag, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  d_flag[b] = fail[b] ? 0 : 1;
  if (fail[b]) d_bits[b] = 0;
}

static int rg_max_len(const kz_batch& bt) { int m = 0; for (int b = 0; b < bt.B; b++) m = std::max(m, bt.h_len[b]); return m; }

size_t kz_range_scratch(int B, int maxN, bool decode) {
  if (decode) return 4096;
  const size_t C = (size_t)std::max(1, (maxN + RG_CHUNK - 1) / RG_CHUNK);
  return (size_t)B * C * (RG_HDR_BYTES + RG_SCRATCH + 20) + (size_t)B * 4 + 8 * 256 + 8192;
}

int64_t kz_range_max_stream_bytes(int n) {
  return (int64_t)kz_align(((size_t)n / RG_CHUNK + 1) * (RG_HDR_BYTES + RG_SCRATCH) + 1024, 256);
}

int kz_stage_range_encode(kz_ctx* ctx, kz_batch& bt, uint8_t* out, int64_t outStride, const int32_t* d_hdrBytes, int64_t* d_bits) {
  const int B = bt.B;
  const int maxN = rg_max_len(bt);
  const int chunks = (maxN + RG_CHUNK - 1) / RG_CHUNK;
  AnsEnc E;
  E.C = std::max(chunks, 1);
  E.chunk = RG_CHUNK; E.hdrStride = RG_HDR_BYTES; E.scrStride = RG_SCRATCH; E.outCap = outStride;
  const size_t NC = (size_t)B * E.C;
  E.hdr = (u8*)kz_arena_alloc(ctx, NC * RG_HDR_BYTES);
  E.scr = (u8*)kz_arena_alloc(ctx, NC * RG_SCRATCH);
  E.hdrBits = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.tailOff = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.tailBits = (u32*)kz_arena_alloc(ctx, NC * 4);
  E.bitOff = (u64*)kz_arena_alloc(ctx, NC * 8);
  int32_t* fail = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  if (!E.hdr || !E.scr || !E.hdrBits || !E.tailOff || !E.tailBits || !E.bitOff || !fail) { snprintf(ctx->err, sizeof(ctx->err), "range encode: arena overflow"); return -KZ_ERR_DEVICE; }
  hipStream_t st = ctx->stream;
  KZ_HIP(hipMemsetAsync(E.hdrBits, 0, NC * 4, st));
  KZ_HIP(hipMemsetAsync(E.tailBits, 0, NC * 4, st));
  KZ_HIP(hipMemsetAsync(fail, 0, (size_t)B * 4, st));
  if (chunks > 0) KZ_LAUNCH(ctx, KID_RANGE_ENC_CHUNK, k_range_enc_chunk, dim3(chunks, B), dim3(64), bt.buf[bt.cur], bt.stride, bt.d_len, E, fail);
  const int rc = kz_chunk_enc_finish(ctx, bt, E, chunks, out, outStride, d_hdrBytes, d_bits, 0);   // no raw form: every non-empty block is chunks
  if (rc) return rc;
  KZ_LAUNCH(ctx, KID_RANGE_ENC_FIN, k_range_enc_fin, dim3((B + 255) / 256), dim3(256), fail, d_bits, bt.d_flag, B);
  KZ_HIP(hipGetLastError());
  return 0;
}

// =================================================================================================
// decode: one wave per block

// the `n` <= 32 bits at bit `pos` of p, MSB first (reads p[pos >> 3 .. + 4])
__device__ __forceinline__ u32 rg_peek(const u8* __restrict__ p, u64 pos, int n) {
  const u64 by = pos >> 3;
  u64 acc = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) acc = (acc << 8) | (u64)p[by + k];
  return (u32)((acc >> (40 - (int)(pos & 7) - n)) & ((1ULL << n) - 1ULL));
}
// InputBitStream.readBits with the block's bit budget: past it the reference throws (the block fails)
struct RgIn { const u8* p; u64 pos, end; bool bad; };
__device__ __forceinline__ u32 rg_get(RgIn& r, int n) {
  if (n == 0 || r.bad) return 0;
  if (r.pos + (u64)n > r.end) { r.bad = true; return 0; }
  const u32 v = rg_peek(r.p, r.pos, n);
  r.pos += (u64)n;
  return v;
}

// (int) ((code - low) / range) of RangeDecoder.java:303: Java's signed 64-bit division (truncating), then the cast to int.
// d = code - low as it wrapped, 2 <= r < 2^63.  The quotient of a valid stream is below 2^15: while |d| < r * 2^16 it comes from the
// hardware's double-precision reciprocal (v_rcp_f64 is good to about 2^-23 relative: the estimate is off by at most one) and is made
// exact with the remainder; beyond that, on damaged input, the 64-bit division proper runs.
__device__ __forceinline__ int32_t rg_quot(u64 d, u64 r) {
  const bool neg = (int64_t)d < 0;
  const u64 a = neg ? (0ULL - d) : d;                             // |d| <= 2^63
  u64 q;
  if ((a >> 16) < r) {
    q = (u64)((double)a * __builtin_amdgcn_rcp((double)r));
    int64_t rem = (int64_t)(a - q * r);
    if (rem < 0) { q--; rem += (int64_t)r; }
    if (rem < 0) { q--; rem += (int64_t)r; }
    if ((u64)rem >= r) { q++; rem -= (int64_t)r; }
    if ((u64)rem >= r) q++;
  } else q = a / r;
  const int64_t sq = neg ? -(int64_t)q : (int64_t)q;
  return (int32_t)(u32)(u64)sq;
}

// f2s[cum .. cum + freq) = symbol (RangeDecoder.java:230-236) by SLOT, as kz_ans.hip fills its table: lane L writes the slots
// [L * scale / 64, (L + 1) * scale / 64), walking the cumulative table from the symbol that owns its first slot.
__device__ __forceinline__ void rg_fill_f2s(const u16* __restrict__ cumf, u8* __restrict__ f2s, int scale, int lane) {
  const int per = scale >> 6;                                     // 4 .. 512: whole groups of four
  const int x0 = lane * per;
  int lo = 0, hi = 256;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int)cumf[mid] <= x0) lo = mid; else hi = mid; }
  int sy = lo;
  int nextAt = (sy + 1 < 256) ? (int)cumf[sy + 1] : 0x7FFFFFFF;
  for (int x = x0; x < x0 + per; x += 4) {
    u32 w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      while (nextAt <= x + k) { sy++; nextAt = (sy + 1 < 256) ? (int)cumf[sy + 1] : 0x7FFFFFFF; }   // sy <= 255: cumf[255] + freq[255] = scale > x + k
      w |= (u32)sy << (8 * k);
    }
    *(u32*)(f2s + x) = w;
  }
}

__global__ __launch_bounds__(64) void k_range_dec(const u8* __restrict__ in, int64_t inStride, const int64_t* __restrict__ d_bitOff,
                                                   const int64_t* __restrict__ d_bitEnd, const int32_t* __restrict__ d_len,
                                                   u8* __restrict__ dst, int64_t stride, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                   long long* __restrict__ endOut) {
  const int b = blockIdx.x, lane = kz_lane();
  const int count = d_len[b];
  if (lane == 0) { d_len2[b] = count; d_flag[b] = 1; }
  if (count <= 0) { if (endOut && lane == 0) endOut[b] = d_bitOff[b]; return; }
  __shared__ __attribute__((aligned(4))) u8 f2s[32768];           // grows only within a block (:226-227): entries at and above the current
  __shared__ u32 symTab[256];                                     // scale are an earlier chunk's, and the chain may read them
  __shared__ u16 freq[256];
  __shared__ u16 cumf[256];
  __shared__ u8 alpha[256];
  RgIn r{in + (int64_t)b * inStride, (u64)d_bitOff[b], (u64)d_bitEnd[b], false};
  u8* o = dst + (int64_t)b * stride;
  int f2sLen = 0;
  bool bad = false;
  int start = 0;
  while (start < count) {
    const int end = min(start + RG_CHUNK, count);
    // ---- decodeHeader :161-239, every lane the same (uniform reads) ----
    __syncthreads();                                              // the previous chunk's table reads are done
    int asz = 0;
    if (rg_get(r, 1) == 0) {
      if (rg_get(r, 1) == 0 && !r.bad) { asz = 256; for (int i = lane; i < 256; i += 64) alpha[i] = (u8)i; }
    } else {
      const int lastMask = (int)rg_get(r, 5);
      for (int i = 0; i <= lastMask && !r.bad; i++) {
        const u32 m = rg_get(r, 8);
        for (int j = 0; j < 8; j++) if (m & (1u << j)) { if (lane == 0) alpha[asz] = (u8)((i << 3) + j); asz++; }
      }
    }
    if (r.bad || asz == 0) { bad = true; break; }                 // :164-165 -> decode() returns startChunk != count
    for (int i = lane; i < 256; i += 64) freq[i] = 0;
    __syncthreads();
    const int lr = 8 + (int)rg_get(r, 3);                         // 8 .. 15: :174-177 cannot throw
    const int scale = 1 << lr;
    {
      int llr = 3;
      while ((1 << llr) <= lr) llr++;
      const int chkSize = (asz >= 64) ? 8 : 6;
      int sum = 0;
      for (int i = 1; i < asz && !bad; i += chkSize) {
        const int logMax = (int)rg_get(r, llr);
        if ((1 << logMax) > scale) { bad = true; break; }         // :192-196
        const int endj = (i + chkSize < asz) ? i + chkSize : asz;
        for (int j = i; j < endj; j++) {
          const int fq = (logMax == 0) ? 1 : 1 + (int)rg_get(r, logMax);
          if (fq >= scale) { bad = true; break; }                 // :204-208
          if (lane == 0) freq[alpha[j]] = (u16)fq;
          sum += fq;
        }
      }
      if (r.bad || scale <= sum) bad = true;                      // :216-221
      if (bad) break;
      if (lane == 0) freq[alpha[0]] = (u16)(scale - sum);
    }
    __syncthreads();
    if (asz == 1) {                                               // :272-279 (f2s is filled all the same: a later, narrower chunk may read it)
      const u8 c = alpha[0];
      for (int i = lane; i < scale; i += 64) f2s[i] = c;
      if (f2sLen < scale) f2sLen = scale;
      for (int i = start + lane; i < end; i += 64) o[i] = c;
      start = end;
      continue;
    }
    // ---- cumFreqs and the reverse mapping :224-236 ----
    {
      u32 cum = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const u32 fv = freq[q * 64 + lane];
        const u32 inc = kz_wave_incl_sum(fv);
        cumf[q * 64 + lane] = (u16)(cum + inc - fv);
        symTab[q * 64 + lane] = (cum + inc - fv) | (fv << 16);
        cum += __shfl(inc, 63, 64);
      }
    }
    __syncthreads();
    rg_fill_f2s(cumf, f2s, scale, lane);
    if (f2sLen < scale) f2sLen = scale;
    __syncthreads();
    // ---- the chain :281-289, decodeByte :300-327 ----
    u64 range = RG_TOP, low = 0;
    u64 code = (u64)rg_get(r, 32) << 28;
    code |= (u64)rg_get(r, 28);
    if (r.bad) { bad = true; break; }
    // the next 28-bit group is requested when the previous one is taken, a byte or more before it is used
    u64 rawNext = (r.pos + 28 <= r.end) ? *(const rg_u64_unaligned*)(r.p + (r.pos >> 3)) : 0ULL;
    u32 outv = 0;
    for (int i = start; i < end && !bad; i++) {
      range >>= lr;
      const int32_t cnt = rg_quot(code - low, range);
      if (cnt < 0 || cnt >= f2sLen) { bad = true; break; }        // ArrayIndexOutOfBoundsException
      const u32 sym = f2s[cnt];
      const u32 ent = symTab[sym];
      const u64 cumFreq = ent & 0xFFFFu, fq = ent >> 16;          // fq == 0: a stale entry's symbol
      low += cumFreq * range;
      range *= fq;
      for (int pass = 0;; pass++) {
        if (((low ^ (low + range)) & RG_MASK) != 0) {
          if ((int64_t)range > (int64_t)RG_BOTTOM) break;
          range = (0ULL - low) & RG_BOTTOM;
        }
        if (pass >= RG_MAX_PASSES || r.pos + 28 > r.end) { bad = true; break; }   // range == 0 reads to the end of the stream and throws there
        const u32 g = (u32)((__builtin_bswap64(rawNext) << (r.pos & 7)) >> 36);
        r.pos += 28;
        rawNext = (r.pos + 28 <= r.end) ? *(const rg_u64_unaligned*)(r.p + (r.pos >> 3)) : 0ULL;
        code = (code << 28) | (u64)g;
        range <<= 28;
        low <<= 28;
      }
      outv = (lane == ((i - start) & 63)) ? sym : outv;
      if (((i - start) & 63) == 63) o[i - 63 + lane] = (u8)outv;  // chunks start at multiples of 32 KiB
    }
    if (bad) break;
    { const int tail = (end - start) & 63; if (lane < tail) o[end - tail + lane] = (u8)outv; }
    start = end;
  }
  if (bad) {                                                      // what the reference never wrote is zero, as the other decoders leave it
    for (int i = start + lane; i < count; i += 64) o[i] = 0;
    if (lane == 0) d_flag[b] = 0;
  }
  if (endOut && lane == 0) endOut[b] = (long long)r.pos;          // bits consumed (EntropyDecoder contract)
}

int kz_stage_range_decode(kz_ctx* ctx, kz_batch& bt, const uint8_t* in, int64_t inStride, const int64_t* d_bitOff, const int64_t* d_bitEnd) {
  const int B = bt.B;
  u8* dst = bt.buf[bt.cur ^ 1];
  KZ_LAUNCH(ctx, KID_RANGE_DEC, k_range_dec, dim3(B), dim3(64), in, inStride, d_bitOff, d_bitEnd, bt.d_len, dst, bt.stride, bt.d_len2, bt.d_flag, ctx->d_endBits);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
