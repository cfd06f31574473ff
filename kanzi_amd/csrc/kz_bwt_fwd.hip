// kz_bwt_fwd.hip -- forward BWT for a batch of blocks on gfx950.
//
// Replaces K/transform/BWTBlockCodec.java:71-128 + K/transform/BWT.java:148-191 +
// K/transform/DivSufSort.java:204-327.  The BWT of a string is unique, so instead of
// imitating DivSufSort's induced sorting (a serial pointer-heavy CPU algorithm) the suffixes are
// sorted the GPU way: prefix doubling where every round is a batched LSD radix sort
// (LDS-staged 256-bin histograms, wave64 ballot match-any ranking, coalesced tile I/O) over the
// still-unsorted suffixes only.  Output convention and the 8 primary indexes follow
// DivSufSort.java:217-224 and :233-325 (primary[k] = ISA[k*step] + 1).
//
// Per block b (n bytes), arrays live in HBM with stride NS elements:
//   key[2] u64, val[2] u32 (suffix index): the compact (still unsorted) suffixes, ping-pong for the radix passes
//   rank u32: ISA as "head slot of the suffix's group", bit 31 = LIVE (group not yet a singleton);  sa u32.
// A round with step h:
//   1. text order (coalesced): every LIVE suffix s emits key = (rank[s] << bitsR) | (rank[s+h] + 1), val = s.
//      Reading rank[s+h] in TEXT order makes both reads sequential; gathering it in SA order (the textbook
//      formulation, and the first version of this file) costs a 128 B line per 4-byte rank and was the largest
//      HBM consumer of the whole encoder (114 GB fetched per launch).  Scanning all n ranks each round costs less
//      than gathering for n/16 live suffixes.
//   2. radix sort of the compact pairs (old group = high key bits, so groups stay contiguous).
//   3. SA order: the members of an old group g occupy the slots g, g+1, ... in sorted order; a new group starts
//      wherever the key changes; rank[val] = new head slot | LIVE, and suffixes whose new group is a singleton are
//      final: sa[slot] = val.  Two max-scans (old-group start index, new-group start index) give the slots.
#include "kz_bwt_fwd.h"
#include <stdlib.h>
#include <algorithm>

#define RS_ITEMS 16
#define RS_TILE (KZ_WG * RS_ITEMS)   // 4096 elements per workgroup
#define RSORT_TILE 16384               // keys per radix tile: a digit run of a tile averages 64 keys = 512 B
#define RSORT_ITEMS (RSORT_TILE / KZ_WG)

// ---------------------------------------------------------------------------------------------
// round 0 keys: the first 7 bytes, zero padded at the end of the text.  A truncated suffix can therefore share a
// group with suffixes that continue with real zero bytes; it is a prefix of all of them, must sort first, and
// does: k_live_emit gives positions past the end of the text the smallest, distinct secondary keys.
__device__ __forceinline__ u64 bw_text_key(const u8* __restrict__ s, int i, int n, int K) {
  // first K bytes as a big-endian number: one unaligned 8-byte load (blocks have >= 4 KiB of slack behind them)
  u64 k = __builtin_bswap64(*(const bw_u64_unaligned*)(s + i)) >> (8 * (8 - K));
  const int rem = n - i;
  if (rem < K) k &= ~0ULL << (8 * (K - rem));                       // zero padding at the end of the text
  return k;
}
// The first LSD pass of round 0 reads the text itself (TextSrc below): the pairs (key, suffix) are never written in
// their initial order, which saves a 12-byte write and a 20-byte read per input byte.
struct TextSrc { const u8* src; int64_t stride; int K; };
__global__ void k_bwt_init(BwtArrays A, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) { A.d_m[b] = A.d_n[b]; A.d_w[b] = 0; }
}

// ---------------------------------------------------------------------------------------------
// radix pass 1/3: per-tile digit histogram (LDS, wave-aggregated via ballot match-any).  BINS = 256 for the LSD passes,
// MSD_BINS for the bucket partition of the later rounds (k_msd_*).
#define MSD_BINS 1024
template <int BINS, bool MSD, bool TEXT>
__device__ __forceinline__ void radix_hist_body(const u64* __restrict__ keyIn, const BwtArrays& A, int shift, TextSrc X) {
  const int b = bw_row_block(A, blockIdx.y);
  const int w0 = MSD ? 0 : A.d_w[b];
  const int m = A.d_m[b] - w0;
  const int tile = blockIdx.x;
  if ((int64_t)tile * RSORT_TILE >= m) return;
  __shared__ u32 hist[BINS];
  for (int i = threadIdx.x; i < BINS; i += KZ_WG) hist[i] = 0;
  __syncthreads();
  const u64* key = keyIn + (int64_t)b * A.NS + w0;
  const int base = tile * RSORT_TILE;
  const int lane = kz_lane();
#pragma unroll 4
  for (int r = 0; r < RSORT_ITEMS; r++) {
    const int idx = base + r * KZ_WG + threadIdx.x;
    const bool valid = idx < m;
    const u32 d = valid ? (u32)(((TEXT ? bw_text_key(X.src + (int64_t)b * X.stride, idx, m, X.K) : key[idx]) >> shift) & (BINS - 1)) : 0;
    // skewed digits (one value for the whole row: high key bytes, runs) would serialise 64 LDS atomics on one
    // address: those rows add once; rows with mixed digits use plain LDS atomics (conflicts only on equal digits)
    const uint64_t vm = kz_ballot(valid);
    const u32 d0 = (u32)__builtin_amdgcn_readfirstlane((int)d);
    if (vm != 0 && kz_ballot(valid && d == d0) == vm) { if (lane == (int)__builtin_ctzll(vm)) atomicAdd(&hist[d0], (u32)__popcll(vm)); }
    else if (valid) atomicAdd(&hist[d], 1u);
  }
  __syncthreads();
  u32* th = A.tileHist + (int64_t)b * A.HS + (int64_t)tile * BINS;
  for (int i = threadIdx.x; i < BINS; i += KZ_WG) th[i] = hist[i];
}
__global__ __launch_bounds__(KZ_WG) void k_radix_hist(const u64* __restrict__ keyIn, BwtArrays A, int shift) { radix_hist_body<256, false, false>(keyIn, A, shift, TextSrc{nullptr, 0, 0}); }
__global__ __launch_bounds__(KZ_WG) void k_radix_hist0(BwtArrays A, TextSrc X) { radix_hist_body<256, false, true>(nullptr, A, 0, X); }
__global__ __launch_bounds__(KZ_WG) void k_msd_hist(const u64* __restrict__ keyIn, BwtArrays A, int shift) { radix_hist_body<MSD_BINS, true, false>(keyIn, A, shift, TextSrc{nullptr, 0, 0}); }

// radix pass 2/3: per block, thread d walks the tiles (coalesced across d) -> exclusive tile
// offsets per digit, then an exclusive scan over digit totals.
__global__ __launch_bounds__(256) void k_radix_scan(BwtArrays A) {
  const int b = bw_row_block(A, blockIdx.x);
  const int m = A.d_m[b] - A.d_w[b];
  const int tiles = (m + RSORT_TILE - 1) / RSORT_TILE;
  __shared__ u32 lds[32];
  u32* h = A.tileHist + (int64_t)b * A.HS;
  u32 run = 0;
  for (int t = 0; t < tiles; t++) {
    u32 v = h[(int64_t)t * 256 + threadIdx.x];
    h[(int64_t)t * 256 + threadIdx.x] = run;
    run += v;
  }
  u32 total;
  u32 ex = kz_wg_excl_sum(run, lds, &total);
  A.digitBase[b * MSD_BINS + threadIdx.x] = ex;
}

// Bucket partition of a later round (k_msd_hist / k_msd_scan / k_msd_scatter): the top bits of the OLD GROUP (a slot of
// the suffix array) split the compact list into buckets of BK_SLOTS slots; a bucket holds at most as many live suffixes
// as it has slots (plus the overhang of its last group), and old groups never span buckets, so a bucket that fits the
// LDS is sorted and applied by one workgroup (k_bucket_sort): one read of the pair instead of six LSD passes.
// Buckets above BK_CAP elements (long runs: one old group of many thousand suffixes) are placed BEHIND the small ones,
// in bucket order, and that window [d_w, d_m) goes through the LSD passes and k_seg_* as before.
// byText: the counts come from k_live_hist, one row of bins per sort tile of the TEXT (a block without live suffixes has none).
__global__ __launch_bounds__(MSD_BINS) void k_msd_scan(BwtArrays A, int byText) {
  const int b = bw_row_block(A, blockIdx.x);
  const int m = A.d_m[b];
  const int tiles = ((byText ? (m > 0 ? A.d_n[b] : 0) : m) + RSORT_TILE - 1) / RSORT_TILE;
  __shared__ u32 lds[32];
  u32* h = A.tileHist + (int64_t)b * A.HS;
  u32 run = 0;
  for (int t = 0; t < tiles; t++) {
    u32 v = h[(int64_t)t * MSD_BINS + threadIdx.x];
    h[(int64_t)t * MSD_BINS + threadIdx.x] = run;
    run += v;
  }
  const bool big = run > BK_CAP;
  u32 mSmall, mBig;
  const u32 exS = kz_wg_excl_sum(big ? 0u : run, lds, &mSmall);
  __syncthreads();
  const u32 exB = kz_wg_excl_sum(big ? run : 0u, lds, &mBig);
  A.digitBase[b * MSD_BINS + threadIdx.x] = big ? mSmall + exB : exS;
  A.bucketCnt[b * MSD_BINS + threadIdx.x] = big ? (run | BK_BIG) : run;
  if (threadIdx.x == 0) { A.d_w[b] = (int32_t)mSmall; A.d_big[b] = (int32_t)mBig; }
}

// radix pass 3/3: stable scatter.  Wave w owns the contiguous sub-tile [w*1024, (w+1)*1024);
// rows of 64 keys are ranked with ballot match-any against per-wave LDS digit counters.  The tile is
// then reordered IN LDS (keys, then values through the same 32 KiB buffer) so that consecutive threads
// store consecutive elements of each digit run: a wave store touches a few 128 B lines instead of up
// to 64 scattered 8 B / 4 B segments (the pass is bound by memory transactions, not bytes).
#define RSC_WAVES 16                      // scatter workgroup: 16 waves x 16 rows of 64 keys = one radix tile
#define RSC_ITEMS (RSORT_TILE / (64 * RSC_WAVES))
#define RSC_WG (64 * RSC_WAVES)
template <int BINS, int NBITS, bool MSD, typename CNT, bool TEXT>
__device__ __forceinline__ void radix_scatter_body(const u64* __restrict__ keyIn, const u32* __restrict__ valIn,
                                                   u64* __restrict__ keyOut, u32* __restrict__ valOut,
                                                   const BwtArrays& A, int shift, TextSrc X) {
  const int b = bw_row_block(A, blockIdx.y);
  const int w0 = MSD ? 0 : A.d_w[b];
  const int m = A.d_m[b] - w0;
  const int tile = blockIdx.x;
  if ((int64_t)tile * RSORT_TILE >= m) return;
  __shared__ CNT cnt[RSC_WAVES][BINS];
  __shared__ u32 gdelta[BINS];       // global slot of the digit's first element of this tile - its tile-local slot
  __shared__ u32 scan[32];
  __shared__ u64 stage[RSORT_TILE];  // 64 KiB: keys, then values
  for (int i = threadIdx.x; i < RSC_WAVES * BINS; i += RSC_WG) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int64_t off = (int64_t)b * A.NS + w0;
  const int wave = threadIdx.x >> 6;
  const int lane = kz_lane();
  const int tbase = tile * RSORT_TILE;
  const int base = tbase + wave * (64 * RSC_ITEMS);
  const int tcount = min(RSORT_TILE, m - tbase);
  const uint64_t lt = kz_lanemask_lt();
  u64 k[RSC_ITEMS]; u32 v[RSC_ITEMS]; u32 dr[RSC_ITEMS];   // dr = digit | (rank<<8), later the tile-local slot
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = base + r * 64 + lane;
    const bool valid = idx < m;
    if (TEXT) {
      k[r] = valid ? bw_text_key(X.src + (int64_t)b * X.stride, idx, m, X.K) : 0;
      v[r] = (u32)idx;
    } else {
      k[r] = valid ? keyIn[off + idx] : 0;
      v[r] = valid ? valIn[off + idx] : 0;
    }
  }
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = base + r * 64 + lane;
    const bool valid = idx < m;
    const u32 d = (u32)((k[r] >> shift) & (BINS - 1));
    // rows holding a single digit value (high key bytes, runs) skip the 8-ballot match-any
    const uint64_t vm = kz_ballot(valid);
    const u32 d0 = (u32)__builtin_amdgcn_readfirstlane((int)d);
    const bool uni = (vm != 0) && (kz_ballot(valid && d == d0) == vm);
    const uint64_t peers = uni ? (valid ? vm : 0ULL) : bw_match<NBITS>(d, valid);
    u32 pre = 0;
    if (valid) pre = cnt[wave][d];
    const u32 rnk = pre + (u32)__popcll(peers & lt);
    // the highest peer lane publishes the new count (all peers read `pre` before: same wave, in order)
    if (valid && (peers >> lane) == 1ULL) cnt[wave][d] = (CNT)(pre + (u32)__popcll(peers));
    dr[r] = d | (rnk << 16);
  }
  __syncthreads();
  {
    u32 tot = 0;
    u32 c[RSC_WAVES];
    const int d = threadIdx.x & (BINS - 1);
#pragma unroll
    for (int w = 0; w < RSC_WAVES; w++) { c[w] = cnt[w][d]; tot += c[w]; }
    u32 total;
    // exclusive scan over the digits (the threads behind them carry zero and are ignored)
    const u32 ts = kz_wg_excl_sum(threadIdx.x < BINS ? tot : 0u, scan, &total);
    if (threadIdx.x < BINS) {
      gdelta[d] = A.digitBase[b * MSD_BINS + d] + A.tileHist[(int64_t)b * A.HS + (int64_t)tile * BINS + d] - ts;
      u32 run = ts;
#pragma unroll
      for (int w = 0; w < RSC_WAVES; w++) { cnt[w][d] = (CNT)run; run += c[w]; }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = base + r * 64 + lane;
    if (idx < m) { const u32 slot = cnt[wave][dr[r] & 0xFFFF] + (dr[r] >> 16); dr[r] = slot; stage[slot] = k[r]; }
  }
  __syncthreads();
  u32 gp[RSC_ITEMS];
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int slot = r * RSC_WG + threadIdx.x;
    if (slot < tcount) {
      const u64 kk = stage[slot];
      gp[r] = gdelta[(u32)((kk >> shift) & (BINS - 1))] + (u32)slot;
      keyOut[off + gp[r]] = kk;
    }
  }
  __syncthreads();
  u32* stageV = (u32*)stage;
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = base + r * 64 + lane;
    if (idx < m) stageV[dr[r]] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int slot = r * RSC_WG + threadIdx.x;
    if (slot < tcount) valOut[off + gp[r]] = stageV[slot];
  }
}
__global__ __launch_bounds__(RSC_WG) void k_radix_scatter(const u64* __restrict__ keyIn, const u32* __restrict__ valIn,
                                                           u64* __restrict__ keyOut, u32* __restrict__ valOut,
                                                           BwtArrays A, int shift) { radix_scatter_body<256, 8, false, u32, false>(keyIn, valIn, keyOut, valOut, A, shift, TextSrc{nullptr, 0, 0}); }
__global__ __launch_bounds__(RSC_WG) void k_radix_scatter0(u64* __restrict__ keyOut, u32* __restrict__ valOut, BwtArrays A, TextSrc X) {
  radix_scatter_body<256, 8, false, u32, true>(nullptr, nullptr, keyOut, valOut, A, 0, X);
}
// The bucket partition need not be stable (k_bucket_sort orders by the whole key, and suffixes with equal keys stay
// one group whatever their order), so the tile-local rank of an element is simply an LDS atomic on its bucket's counter.
#define MSD_NONE 0xFFFFFFFFu
// one row of 64 elements takes its positions in the tile's bucket counters: d = the lane's bucket, returns the position inside
// (tile, bucket), MSD_NONE for a lane without an element.  A row of one bucket costs one atomic.
__device__ __forceinline__ u32 msd_tile_place(u32* cnt, u32 d, bool valid, int lane, uint64_t lt) {
  const uint64_t vm = kz_ballot(valid);
  if (vm == 0) return MSD_NONE;
  const int l0 = (int)__builtin_ctzll(vm);
  const u32 d0 = (u32)__builtin_amdgcn_readlane((int)d, l0);
  u32 pos = MSD_NONE;
  if (kz_ballot(valid && d == d0) == vm) {
    u32 basePos = 0;
    if (lane == l0) basePos = atomicAdd(&cnt[d0], (u32)__popcll(vm));
    basePos = (u32)__builtin_amdgcn_readlane((int)basePos, l0);
    if (valid) pos = basePos + (u32)__popcll(vm & lt);
  } else if (valid) pos = atomicAdd(&cnt[d], 1u);
  return pos;
}
// ... and the tile leaves (k_msd_scatter, k_live_scatter): exclusive scan of the tile's bucket counts, gdelta = the bucket's global
// slot for this tile (digitBase + the scanned tileHist) - its tile-local slot, then keys and values through the LDS stage so that
// consecutive threads store consecutive elements of a bucket's run.  dr[r] = position inside (tile, bucket) or MSD_NONE.
__device__ __forceinline__ void msd_tile_flush(const u64 (&k)[RSC_ITEMS], const u32 (&v)[RSC_ITEMS], u32 (&dr)[RSC_ITEMS], int shift,
                                               u64* __restrict__ keyOut, u32* __restrict__ valOut, const BwtArrays& A, int b, int tile,
                                               u32* cnt, u32* gdelta, u32* scan, u64* stage) {
  __syncthreads();
  u32 tcount;
  {
    const u32 tot = cnt[threadIdx.x];
    const u32 ts = kz_wg_excl_sum(tot, scan, &tcount);
    gdelta[threadIdx.x] = A.digitBase[b * MSD_BINS + threadIdx.x] + A.tileHist[(int64_t)b * A.HS + (int64_t)tile * MSD_BINS + threadIdx.x] - ts;
    cnt[threadIdx.x] = ts;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    if (dr[r] != MSD_NONE) { const u32 slot = cnt[(u32)(k[r] >> shift) & (MSD_BINS - 1)] + dr[r]; dr[r] = slot; stage[slot] = k[r]; }
  }
  __syncthreads();
  u32 gp[RSC_ITEMS];
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const u32 slot = (u32)r * RSC_WG + threadIdx.x;
    if (slot < tcount) {
      const u64 kk = stage[slot];
      gp[r] = gdelta[(u32)(kk >> shift) & (MSD_BINS - 1)] + slot;
      keyOut[gp[r]] = kk;
    }
  }
  __syncthreads();
  u32* stageV = (u32*)stage;
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    if (dr[r] != MSD_NONE) stageV[dr[r]] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const u32 slot = (u32)r * RSC_WG + threadIdx.x;
    if (slot < tcount) valOut[gp[r]] = stageV[slot];
  }
}
__global__ __launch_bounds__(RSC_WG) void k_msd_scatter(const u64* __restrict__ keyIn, const u32* __restrict__ valIn,
                                                         u64* __restrict__ keyOut, u32* __restrict__ valOut,
                                                         BwtArrays A, int shift) {
  const int b = bw_row_block(A, blockIdx.y);
  const int m = A.d_m[b];
  const int tile = blockIdx.x;
  if ((int64_t)tile * RSORT_TILE >= m) return;
  __shared__ u32 cnt[MSD_BINS];
  __shared__ u32 gdelta[MSD_BINS];
  __shared__ u32 scan[32];
  __shared__ u64 stage[RSORT_TILE];  // 128 KiB: keys, then values
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t off = (int64_t)b * A.NS;
  const int lane = kz_lane();
  const int tbase = tile * RSORT_TILE;
  const uint64_t lt = kz_lanemask_lt();
  u64 k[RSC_ITEMS]; u32 v[RSC_ITEMS]; u32 dr[RSC_ITEMS];
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = tbase + r * RSC_WG + threadIdx.x;
    const bool valid = idx < m;
    k[r] = valid ? keyIn[off + idx] : 0;
    v[r] = valid ? valIn[off + idx] : 0;
  }
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int idx = tbase + r * RSC_WG + threadIdx.x;
    dr[r] = msd_tile_place(cnt, (u32)(k[r] >> shift) & (MSD_BINS - 1), idx < m, lane, lt);
  }
  msd_tile_flush(k, v, dr, shift, keyOut + off, valOut + off, A, b, tile, cnt, gdelta, scan, stage);
}

// ---------------------------------------------------------------------------------------------
// step 3 (SA order, after the sort).  g(c) = old group head slot = key >> gshift (gshift >= 64: one group, slot 0).
__device__ __forceinline__ u32 bw_group(u64 k, int gshift) { return gshift >= 64 ? 0u : (u32)(k >> gshift); }

// Wave w of a tile owns the 1024 consecutive sorted elements [w*1024, (w+1)*1024) as 16 rows of 64 (coalesced).
// Loads the keys, returns per row the ballots "key differs from its predecessor" (hb) and "old group differs" (sb).
__device__ __forceinline__ void bw_row_flags(const u64* __restrict__ key, int base, int m, int gshift, int lane,
                                             u64 (&k)[RS_ITEMS], uint64_t (&hb)[RS_ITEMS], uint64_t (&sb)[RS_ITEMS]) {
  u64 prevRowLast = (base > 0 && base <= m) ? key[base - 1] : 0;      // uniform
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    const int c = base + r * 64 + lane;
    k[r] = (c < m) ? key[c] : 0;
    u64 prev = __shfl_up(k[r], 1, 64);
    if (lane == 0) prev = prevRowLast;
    const bool valid = c < m;
    const bool head = valid && (c == 0 || k[r] != prev);
    const bool seg = head && (c == 0 || bw_group(k[r], gshift) != bw_group(prev, gshift));
    hb[r] = kz_ballot(head);
    sb[r] = kz_ballot(seg);
    prevRowLast = __shfl(k[r], 63, 64);
  }
}

// per tile: (last index+1 where the old group changes, last index+1 where the key changes)
__global__ __launch_bounds__(KZ_WG) void k_seg_reduce(const u64* __restrict__ keyS, BwtArrays A, int gshift) {
  const int b = bw_row_block(A, blockIdx.y);
  const int w0 = A.d_w[b];
  const int m = A.d_m[b] - w0;
  const int tile = blockIdx.x;
  if ((int64_t)tile * RS_TILE >= m) return;
  __shared__ u32 wS[4], wH[4];
  const u64* key = keyS + (int64_t)b * A.NS + w0;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const int base = tile * RS_TILE + wave * (64 * RS_ITEMS);
  u64 k[RS_ITEMS]; uint64_t hb[RS_ITEMS], sb[RS_ITEMS];
  bw_row_flags(key, base, m, gshift, lane, k, hb, sb);
  u32 ms = 0, mh = 0;
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    if (hb[r]) mh = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(hb[r])) + 1;
    if (sb[r]) ms = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(sb[r])) + 1;
  }
  if (lane == 0) { wS[wave] = ms; wH[wave] = mh; }
  __syncthreads();
  if (threadIdx.x == 0) {
    A.tileA[(int64_t)b * A.T + tile] = max(max(wS[0], wS[1]), max(wS[2], wS[3]));
    A.tileB[(int64_t)b * A.T + tile] = max(max(wH[0], wH[1]), max(wH[2], wH[3]));
  }
}
// per block: exclusive max-scans over the tiles -- one wave per block
__global__ void k_seg_scan(BwtArrays A) {
  const int b = bw_row_block(A, blockIdx.x);
  const int m = A.d_m[b] - A.d_w[b];
  const int tiles = (m + RS_TILE - 1) / RS_TILE;
  u32* ta = A.tileA + (int64_t)b * A.T;
  u32* tb = A.tileB + (int64_t)b * A.T;
  u32 ca = 0, cb = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int i = base + threadIdx.x;
    const u32 va = (i < tiles) ? ta[i] : 0, vb = (i < tiles) ? tb[i] : 0;
    const u32 ia = kz_wave_incl_max(va), ib = kz_wave_incl_max(vb);
    u32 ea = __shfl_up(ia, 1, 64), eb = __shfl_up(ib, 1, 64);
    if (threadIdx.x == 0) { ea = 0; eb = 0; }
    ea = ea > ca ? ea : ca; eb = eb > cb ? eb : cb;
    if (i < tiles) { ta[i] = ea; tb[i] = eb; }
    const u32 la = __shfl(ia, 63, 64), lb = __shfl(ib, 63, 64);
    ca = ca > la ? ca : la; cb = cb > lb ? cb : lb;
  }
}
// apply: slot = g + (c - segment start); new rank = g + (new-group start - segment start); LIVE unless the new
// group is a singleton, in which case the suffix is final
__global__ __launch_bounds__(KZ_WG) void k_seg_apply(const u64* __restrict__ keyS, const u32* __restrict__ valS, BwtArrays A, int gshift) {
  const int b = bw_row_block(A, blockIdx.y);
  const int w0 = A.d_w[b];
  const int m = A.d_m[b] - w0;
  const int tile = blockIdx.x;
  if ((int64_t)tile * RS_TILE >= m) return;
  __shared__ u32 wS[4], wH[4];
  const int64_t off = (int64_t)b * A.NS;
  const u64* key = keyS + off + w0;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const int base = tile * RS_TILE + wave * (64 * RS_ITEMS);
  u64 k[RS_ITEMS]; uint64_t hb[RS_ITEMS], sb[RS_ITEMS];
  bw_row_flags(key, base, m, gshift, lane, k, hb, sb);
  u32 ms = 0, mh = 0;
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    if (hb[r]) mh = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(hb[r])) + 1;
    if (sb[r]) ms = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(sb[r])) + 1;
  }
  if (lane == 0) { wS[wave] = ms; wH[wave] = mh; }
  __syncthreads();
  // carry into this wave: the tile's carry and the previous waves of the tile ("index + 1", 0 = none)
  u32 carS = A.tileA[(int64_t)b * A.T + tile], carH = A.tileB[(int64_t)b * A.T + tile];
  for (int w = 0; w < wave; w++) { carS = max(carS, wS[w]); carH = max(carH, wH[w]); }
  u32* rank = A.rank + off;
  u32* sa = A.sa + off;
  const u32* val = valS + off + w0;
  const uint64_t le = kz_lanemask_lt() | (1ULL << lane);
  const u64 afterLast = (base + 64 * RS_ITEMS < m) ? key[base + 64 * RS_ITEMS] : 0;   // uniform
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    const int rowBase = base + r * 64;
    const int c = rowBase + lane;
    const uint64_t hbl = hb[r] & le, sbl = sb[r] & le;
    const u32 hh = hbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(hbl)) : carH - 1;   // index of the new group's first element
    const u32 ss = sbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(sbl)) : carS - 1;   // index of the old group's first element
    // key of the next element: next lane / first lane of the next row / first key behind the wave's chunk
    u64 nextk = __shfl_down(k[r], 1, 64);
    const u64 nextRowFirst = (r + 1 < RS_ITEMS) ? __shfl(k[(r + 1 < RS_ITEMS) ? r + 1 : r], 0, 64) : afterLast;
    if (lane == 63) nextk = nextRowFirst;
    if (c < m) {
      const u32 g = bw_group(k[r], gshift);
      const bool headC = hh == (u32)c;
      const bool headN = (c + 1 >= m) || (nextk != k[r]);
      const u32 sv = val[c];
      const bool live = !(headC && headN);
      // the first new group of an old group keeps the old head slot: while it stays LIVE its members' ranks (g | LIVE since the
      // round before) do not change, and the random 4-byte store is saved (not in the first round: ranks are unwritten then)
      if (!(live && hh == ss && gshift < 64)) rank[sv] = (g + (hh - ss)) | (live ? BW_LIVE : 0u);
      if (!live) sa[g + ((u32)c - ss)] = sv;
    }
    if (hb[r]) carH = (u32)(rowBase + 63 - (int)__builtin_clzll(hb[r])) + 1;
    if (sb[r]) carS = (u32)(rowBase + 63 - (int)__builtin_clzll(sb[r])) + 1;
  }
}

// ---------------------------------------------------------------------------------------------
// One bucket of a later round whose longest old group is above BK_GMAX (flagged by k_bucket_count*), start to finish in one
// workgroup: load the bucket's pairs, LSD radix sort them in LDS by (old group, secondary key), then do what k_seg_reduce /
// k_seg_apply do for the sorted run.  An element is one u64: (group - bucket base : BK_BITS | r2 : bitsR | suffix : bitsG),
// 58 bits for 4 MiB blocks.  Wave w owns the contiguous rows [w*R, (w+1)*R) of 64 elements; between passes the elements
// live in registers, the LDS buffer is only the exchange (48 KiB + 16 KiB of u16 counters, 64 VGPRs: two workgroups per CU).
static_assert(RSC_WG == MSD_BINS, "k_msd_scatter geometry");

template <int WAVES, int ROWS>
__device__ __forceinline__ void bucket_body(const u64* __restrict__ keyS, const u32* __restrict__ valS, const BwtArrays& A, int bitsR, int bitsG) {
  const int b = bw_row_block(A, blockIdx.y);
  const u32 d = blockIdx.x;
  const u32 bc0 = A.bucketCnt[b * MSD_BINS + d];
  if ((bc0 & (BK_SORT | BK_BIG)) != BK_SORT) return;          // only the buckets k_bucket_count left behind
  const u32 bc = bc0 & ~BK_SORT;
  const int cnt = (int)bc;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  __shared__ u64 buf[WAVES * ROWS * 64];
  __shared__ uint16_t cw[WAVES][BK_DBINS];                     // per-wave digit counts, then bucket-local slots
  __shared__ u32 wsum[BK_DBINS / 64];
  __shared__ u32 wS[WAVES], wH[WAVES];
  __shared__ int skip[8];
  const int64_t off = (int64_t)b * A.NS;
  const u32 bo = A.digitBase[b * MSD_BINS + d];
  const int rows = (cnt + 63) >> 6;
  const int R = (rows + WAVES - 1) / WAVES;                    // rows per wave, 1..ROWS (uniform)
  const int base = wave * R * 64;
  const uint64_t lt = kz_lanemask_lt();
  const u64 kbase = (u64)d << (bitsR + BK_BITS);
  u64 k[ROWS]; u32 dr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int idx = base + r * 64 + lane;
    k[r] = ~0ULL;
    if (r < R && idx < cnt) k[r] = ((keyS[off + bo + idx] - kbase) << bitsG) | (u64)valS[off + bo + idx];
  }
  // The pass loop below and the one of tr_sort_body (kz_bwt_trie.hip) are the same LSD pass in two texts, and stay two: this one keeps
  // a digit's per-wave counts in registers (c[][]) between the barriers, that one reads them from LDS twice because k_tr_sort /
  // k_trk_sort have no registers left.  One shared loop was measured in both forms (profiles/bwt_fwd_refactor.txt): re-reading costs
  // k_bucket_sort 2.5 %, keeping the counts costs the trie sorts 28 to 68 B more scratch per lane.  A change to one is due in the other.
  {
    if (threadIdx.x < 8) skip[threadIdx.x] = 0;
    const int keyBits = bitsR + BK_BITS;
    const int passes = (keyBits + BK_DBITS - 1) / BK_DBITS;
    for (int p = 0; p < passes; p++) {
      const int shift = bitsG + BK_DBITS * p;
      for (int i = threadIdx.x; i < WAVES * BK_DBINS / 2; i += WAVES * 64) ((u32*)&cw[0][0])[i] = 0;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          const bool valid = idx < cnt;
          const u32 dg = (u32)(k[r] >> shift) & (BK_DBINS - 1);
          const uint64_t vm = kz_ballot(valid);
          if (vm == 0) continue;                               // rows behind the bucket's last element (uniform)
          const u32 d0 = (u32)__builtin_amdgcn_readfirstlane((int)dg);
          const bool uni = kz_ballot(valid && dg == d0) == vm;
          const uint64_t peers = uni ? (valid ? vm : 0ULL) : bw_match<BK_DBITS>(dg, valid);
          u32 pre = 0;
          if (valid) pre = cw[wave][dg];
          const u32 rnk = pre + (u32)__popcll(peers & lt);
          if (valid && (peers >> lane) == 1ULL) cw[wave][dg] = (uint16_t)(pre + (u32)__popcll(peers));
          dr[r] = dg | (rnk << 16);
        }
      }
      __syncthreads();
      // digit totals and their exclusive scan: thread t owns the digits t, t + WAVES*64, ...
      constexpr int DPT = (BK_DBINS + WAVES * 64 - 1) / (WAVES * 64);
      u32 c[DPT][WAVES]; u32 tot[DPT]; u32 mine = 0;
#pragma unroll
      for (int q = 0; q < DPT; q++) {
        const int dg = threadIdx.x * DPT + q;                  // consecutive digits per thread: a plain scan order
        tot[q] = 0;
        if (dg < BK_DBINS) {
#pragma unroll
          for (int w = 0; w < WAVES; w++) { c[q][w] = cw[w][dg]; tot[q] += c[q][w]; }
          if (tot[q] == (u32)cnt) skip[p] = 1;                 // one digit value for the whole bucket: nothing moves
        }
        mine += tot[q];
      }
      const u32 inc = kz_wave_incl_sum(mine);
      if (lane == 63 && wave < BK_DBINS / 64) wsum[wave] = inc;
      __syncthreads();
      if (skip[p]) continue;                                   // uniform
      {
        u32 run = inc - mine;
        for (int w = 0; w < wave && w < BK_DBINS / 64; w++) run += wsum[w];
#pragma unroll
        for (int q = 0; q < DPT; q++) {
          const int dg = threadIdx.x * DPT + q;
          if (dg < BK_DBINS) {
#pragma unroll
            for (int w = 0; w < WAVES; w++) { cw[w][dg] = (uint16_t)run; run += c[q][w]; }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          if (idx < cnt) buf[cw[wave][dr[r] & 0xFFFF] + (dr[r] >> 16)] = k[r];
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          if (idx < cnt) k[r] = buf[idx];
        }
      }
      __syncthreads();
    }
    // sorted: neighbours through the LDS buffer
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      if (r < R) {
        const int idx = base + r * 64 + lane;
        if (idx < cnt) buf[idx] = k[r];
      }
    }
    __syncthreads();
  }
  // groups (NOT shared with tr_sort_body's, on purpose: here the rows' ballots stay in registers between the two loops, there they
  // are computed twice -- k_tr_sort / k_trk_sort have no registers left for them: see the comment there)
  uint64_t hb[ROWS], sb[ROWS];
  u32 ms = 0, mh = 0;
  const int gsh = bitsG + bitsR;
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    hb[r] = 0; sb[r] = 0;
    if (r < R) {
      const int idx = base + r * 64 + lane;
      const bool valid = idx < cnt;
      const u64 prev = (valid && idx > 0) ? buf[idx - 1] : 0;
      const bool head = valid && (idx == 0 || (k[r] >> bitsG) != (prev >> bitsG));
      const bool seg = head && (idx == 0 || (k[r] >> gsh) != (prev >> gsh));
      hb[r] = kz_ballot(head);
      sb[r] = kz_ballot(seg);
      if (hb[r]) mh = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(hb[r])) + 1;
      if (sb[r]) ms = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(sb[r])) + 1;
    }
  }
  u32 carS = 0, carH = 0;
  {
    if (lane == 0) { wS[wave] = ms; wH[wave] = mh; }
    __syncthreads();
    for (int w = 0; w < wave; w++) { carS = max(carS, wS[w]); carH = max(carH, wH[w]); }
  }
  u32* rank = A.rank + off;
  u32* sa = A.sa + off;
  const uint64_t le = lt | (1ULL << lane);
  const u64 vmask = (1ULL << bitsG) - 1ULL;
  const u32 gbase = d << BK_BITS;
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    if (r < R) {
      const int rowBase = base + r * 64;
      const int idx = rowBase + lane;
      const uint64_t hbl = hb[r] & le, sbl = sb[r] & le;
      const u32 hh = hbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(hbl)) : carH - 1;
      const u32 ss = sbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(sbl)) : carS - 1;
      if (idx < cnt) {
        const u64 nextk = (idx + 1 < cnt) ? buf[idx + 1] : 0;
        const bool headC = hh == (u32)idx;
        const bool headN = (idx + 1 >= cnt) || ((nextk >> bitsG) != (k[r] >> bitsG));
        const bool live = !(headC && headN);
        const u32 g = gbase + (u32)(k[r] >> gsh);
        const u32 sv = (u32)(k[r] & vmask);
        if (!(live && hh == ss)) rank[sv] = (g + (hh - ss)) | (live ? BW_LIVE : 0u);     // see k_seg_apply
        if (!live) sa[g + ((u32)idx - ss)] = sv;
      }
      if (hb[r]) carH = (u32)(rowBase + 63 - (int)__builtin_clzll(hb[r])) + 1;
      if (sb[r]) carS = (u32)(rowBase + 63 - (int)__builtin_clzll(sb[r])) + 1;
    }
  }
}
__global__ __launch_bounds__(1024, 8) void k_bucket_sort(const u64* __restrict__ keyS, const u32* __restrict__ valS, BwtArrays A, int bitsR, int bitsG) {
  bucket_body<16, BK_CAP / 1024>(keyS, valS, A, bitsR, bitsG);
}

// ---------------------------------------------------------------------------------------------
// The same job without sorting.  What the apply step needs of a suffix is only, among the members of its old group,
// how many have a smaller secondary key (rk) and how many the same one (eq): the new group starts rk slots behind the
// old head, it is a singleton iff eq == 1, and then the suffix's final slot is head + rk.  So the bucket is only
// PARTITIONED by old group (LDS atomics on one counter per slot of the bucket: order inside a group is irrelevant), and
// every element then walks the members of its group.  Groups are small where this is used (a handful of suffixes
// sharing 7, 14, ... bytes); a bucket holding a group above BK_GMAX is left to k_bucket_sort (flag BK_SORT).
template <int WAVES, int ROWS, int LO, int HI, typename CNT>
__device__ __forceinline__ void bucket_count_body(const u64* __restrict__ keyS, const u32* __restrict__ valS, const BwtArrays& A, int bitsR, int bitsG, u32 gmax) {
  const int b = bw_row_block(A, blockIdx.y);
  const u32 d = blockIdx.x;
  const u32 bc = A.bucketCnt[b * MSD_BINS + d];
  if (bc <= (u32)LO || bc > (u32)HI) return;
  const int cnt = (int)bc;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const bool tiny = LO == 0 && cnt <= 64;
  if (tiny && wave != 0) return;
  const int64_t off = (int64_t)b * A.NS;
  const u32 bo = A.digitBase[b * MSD_BINS + d];
  u32* rank = A.rank + off;
  u32* sa = A.sa + off;
  const u32 gbase = d << BK_BITS;
  const u32 rmask = (1u << bitsR) - 1u;
  constexpr int WG = WAVES * 64;
  if (tiny) {
    const bool valid = lane < cnt;
    const u64 key = valid ? keyS[off + bo + lane] : ~0ULL;
    const u32 sv = valid ? valS[off + bo + lane] : 0u;
    const u32 gv = (u32)(key >> bitsR), rv = (u32)key & rmask;
    u32 rk = 0, eq = 0;
    for (int j = 0; j < cnt; j++) {
      const u32 gj = (u32)__builtin_amdgcn_readlane((int)gv, j), rj = (u32)__builtin_amdgcn_readlane((int)rv, j);
      if (gj == gv) { rk += (rj < rv) ? 1u : 0u; eq += (rj == rv) ? 1u : 0u; }
    }
    if (valid) {
      const bool live = eq > 1;
      if (!(live && rk == 0)) rank[sv] = (gv + rk) | (live ? BW_LIVE : 0u);               // see k_seg_apply
      if (!live) sa[gv + rk] = sv;
    }
    return;
  }
  __shared__ u64 buf[WAVES * ROWS * 64];
  __shared__ CNT start[BK_SLOTS];
  __shared__ u32 wsum[WAVES];
  __shared__ u32 gmaxS;
  for (int i = threadIdx.x; i < BK_SLOTS; i += WG) start[i] = 0;
  if (threadIdx.x == 0) gmaxS = 0;
  __syncthreads();
  const u64 kbase = (u64)d << (bitsR + BK_BITS);
  u64 k[ROWS]; u32 pos[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int idx = r * WG + threadIdx.x;
    k[r] = 0; pos[r] = 0;
    if (idx < cnt) {
      k[r] = ((keyS[off + bo + idx] - kbase) << bitsG) | (u64)valS[off + bo + idx];
      pos[r] = (u32)atomicAdd(&start[(u32)(k[r] >> (bitsG + bitsR))], (CNT)1);
    }
  }
  __syncthreads();
  {                                                            // exclusive scan over the slots: BK_SLOTS / WG consecutive per thread
    constexpr int SPT = BK_SLOTS / WG;
    u32 c[SPT]; u32 mine = 0, gm = 0;
#pragma unroll
    for (int q = 0; q < SPT; q++) { c[q] = start[threadIdx.x * SPT + q]; mine += c[q]; gm = max(gm, c[q]); }
    const u32 inc = kz_wave_incl_sum(mine);
    if (lane == 63) wsum[wave] = inc;
    if (gm > gmax) atomicMax(&gmaxS, gm);
    __syncthreads();
    u32 run = inc - mine;
    for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
    for (int q = 0; q < SPT; q++) { start[threadIdx.x * SPT + q] = (CNT)run; run += c[q]; }
  }
  __syncthreads();
  if (gmaxS > gmax) {                                        // a long group: the sorting kernel takes this bucket
    if (threadIdx.x == 0) A.bucketCnt[b * MSD_BINS + d] = bc | BK_SORT;
    return;
  }
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int idx = r * WG + threadIdx.x;
    if (idx < cnt) buf[(u32)start[(u32)(k[r] >> (bitsG + bitsR))] + pos[r]] = k[r];
  }
  __syncthreads();
  const u64 vmask = (1ULL << bitsG) - 1ULL;
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int idx = r * WG + threadIdx.x;                      // position in group order: a wave reads a few neighbouring groups
    if (idx < cnt) {
      const u64 e = buf[idx];
      const u32 grel = (u32)(e >> (bitsG + bitsR));
      const u32 rv = (u32)(e >> bitsG) & rmask;
      const int gs = (int)start[grel];
      const int ge = (grel + 1 < (u32)BK_SLOTS) ? (int)start[grel + 1] : cnt;
      u32 rk = 0, eq = 0;
      int j = gs;
      for (; j + 4 <= ge; j += 4) {                            // four independent LDS reads in flight
        const u64 e0 = buf[j], e1 = buf[j + 1], e2 = buf[j + 2], e3 = buf[j + 3];
        const u32 r0 = (u32)(e0 >> bitsG) & rmask, r1 = (u32)(e1 >> bitsG) & rmask, r2_ = (u32)(e2 >> bitsG) & rmask, r3 = (u32)(e3 >> bitsG) & rmask;
        rk += (r0 < rv) + (r1 < rv) + (r2_ < rv) + (r3 < rv);
        eq += (r0 == rv) + (r1 == rv) + (r2_ == rv) + (r3 == rv);
      }
      for (; j < ge; j++) {
        const u32 rj = (u32)(buf[j] >> bitsG) & rmask;
        rk += (rj < rv) ? 1u : 0u; eq += (rj == rv) ? 1u : 0u;
      }
      const u32 sv = (u32)(e & vmask);
      const u32 g = gbase + grel;
      const bool live = eq > 1;
      if (!(live && rk == 0)) rank[sv] = (g + rk) | (live ? BW_LIVE : 0u);
      if (!live) sa[g + rk] = sv;
    }
  }
}
__global__ __launch_bounds__(256) void k_bucket_count_s(const u64* __restrict__ keyS, const u32* __restrict__ valS, BwtArrays A, int bitsR, int bitsG, u32 gmax) {
  bucket_count_body<4, BK_SMALL / 256, 0, BK_SMALL, u32>(keyS, valS, A, bitsR, bitsG, gmax);
}
__global__ __launch_bounds__(1024) void k_bucket_count(const u64* __restrict__ keyS, const u32* __restrict__ valS, BwtArrays A, int bitsR, int bitsG, u32 gmax) {
  bucket_count_body<16, BK_CAP / 1024, BK_SMALL, BK_CAP, u32>(keyS, valS, A, bitsR, bitsG, gmax);
}

// ---------------------------------------------------------------------------------------------
// step 1 (text order): compact the LIVE suffixes and build their keys from sequential rank reads
// The compact list need not be in text order (its only readers partition it by group: k_msd_* / the key trie round), so a tile
// reserves its slice with ONE returning atomic on the block's counter instead of a count kernel + a scan kernel + a second read of
// every rank (k_live_count / k_live_scan until round 4: 36 ms and 122 GB of rank reads per 8 GiB).  Inside a tile the order stays
// the text order.  tileLive[tile] = live suffixes of the tile after the previous round (0 stays 0: suffixes only become final).
__global__ __launch_bounds__(KZ_WG) void k_live_emit(u64* __restrict__ keyN, u32* __restrict__ valN, BwtArrays A, int h, int bitsR, int first, const int32_t* __restrict__ lazyMeta) {
  const int b = bw_row_block(A, blockIdx.y);
  const int n = A.d_n[b];
  const int tile = blockIdx.x;
  if ((int64_t)tile * RS_TILE >= n) return;
  if (lazyMeta && lazyMeta[(int64_t)b * TR_META] == 256 && lazyMeta[(int64_t)b * TR_META + 18] == 0 && lazyMeta[(int64_t)b * TR_META + 20] == 0) {
    // round 0 left no live suffix in this block and stored no ranks (k_tr_sort, lazy ranks): nothing to read, nothing to emit
    if (threadIdx.x == 0) A.tileLive[(int64_t)b * A.T + tile] = 0;
    return;
  }
  if (!first && A.tileLive[(int64_t)b * A.T + tile] == 0) return;     // nothing left here: neither read nor written
  __shared__ u32 rowCnt[RS_ITEMS * 4 + 1];   // live suffixes per (wave, row), then exclusive prefix
  __shared__ u32 tileBase;
  const int64_t off = (int64_t)b * A.NS;
  const u32* rank = A.rank + off;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  // wave w owns the 1024 consecutive suffixes [w*1024, (w+1)*1024): rows of 64 -> every access is coalesced
  const int base = tile * RS_TILE + wave * (64 * RS_ITEMS);
  u32 rk[RS_ITEMS];
  uint64_t bal[RS_ITEMS];
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    const int s = base + r * 64 + lane;
    rk[r] = (s < n) ? rank[s] : 0u;
    bal[r] = kz_ballot((rk[r] & BW_LIVE) != 0);
    if (lane == 0) rowCnt[wave * RS_ITEMS + r] = (u32)__popcll(bal[r]);
  }
  __syncthreads();
  if (threadIdx.x < 64) {                      // exclusive scan of the 64 (wave,row) counts by one wave
    const u32 v = rowCnt[threadIdx.x];
    const u32 inc = kz_wave_incl_sum(v);
    rowCnt[threadIdx.x] = inc - v;
    if (threadIdx.x == 63) {
      const u32 tot = inc;
      A.tileLive[(int64_t)b * A.T + tile] = tot;
      tileBase = tot ? (u32)atomicAdd(&A.d_m2[b], (int32_t)tot) : 0u;
    }
  }
  __syncthreads();
  const u32 tbase = tileBase;
  const uint64_t lt = kz_lanemask_lt();
  const u32 hcap = (u32)min(h, n);
#pragma unroll
  for (int r = 0; r < RS_ITEMS; r++) {
    if (rk[r] & BW_LIVE) {
      const int s = base + r * 64 + lane;
      const int64_t j = (int64_t)s + h;
      // positions past the end (s + h >= n): n - s in [1, min(h, n)], smaller for the shorter suffix and below every real rank
      const u64 r2 = (j < n) ? (u64)(rank[j] & ~BW_LIVE) + (u64)hcap + 1ULL : (u64)(n - s);
      const u32 pos = tbase + rowCnt[wave * RS_ITEMS + r] + (u32)__popcll(bal[r] & lt);
      keyN[off + pos] = ((u64)(rk[r] & ~BW_LIVE) << bitsR) | r2;
      valN[off + pos] = (u32)s;
    }
  }
}

// The bucket partition of the next round straight from the ranks: where the next round takes the bucket path, the text-order list
// above has no reader but k_msd_hist / k_msd_scatter, and 32 of the 64 bytes the three kernels move per live suffix only hand it
// over.  k_live_hist (end of a round) counts the live suffixes of a sort tile of RSORT_TILE TEXT positions per bucket of their group
// -- the row of bins k_msd_scan takes -- and k_live_scatter (start of the next round, behind the scan) reads the tile's ranks again,
// builds k_live_emit's element and places it with k_msd_scatter's machinery.  Thread t of 1024 owns the positions tbase + r * 1024 +
// t: rows r = 4q .. 4q + 3 are the RS_TILE sub-tile q of tileLive, whose dead ones are neither read nor counted.
static_assert(RSORT_TILE == 4 * RS_TILE && RSC_ITEMS == 16, "k_live_hist / k_live_scatter: four rows of a thread per sub-tile");
// which of the tile's four sub-tiles to read (bit q), by the round before; a sub-tile behind the end of the text has no tileLive entry
__device__ __forceinline__ u32 live_subtiles(const BwtArrays& A, int b, int tile, int n, int first) {
  u32 m = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int sub = tile * 4 + q;
    if ((int64_t)sub * RS_TILE < n && (first || A.tileLive[(int64_t)b * A.T + sub] != 0)) m |= 1u << q;
  }
  return m;
}
__global__ __launch_bounds__(RSC_WG) void k_live_hist(BwtArrays A, int first, const int32_t* __restrict__ lazyMeta) {
  const int b = bw_row_block(A, blockIdx.y);
  const int n = A.d_n[b];
  const int tile = blockIdx.x;
  if ((int64_t)tile * RSORT_TILE >= n) return;
  u32* th = A.tileHist + (int64_t)b * A.HS + (int64_t)tile * MSD_BINS;
  u32* tl = A.tileLive + (int64_t)b * A.T + tile * 4;
  const bool inText = threadIdx.x < 4 && (int64_t)(tile * 4 + (int)threadIdx.x) * RS_TILE < n;
  if (lazyMeta && lazyMeta[(int64_t)b * TR_META] == 256 && lazyMeta[(int64_t)b * TR_META + 18] == 0 && lazyMeta[(int64_t)b * TR_META + 20] == 0) {
    // round 0 left no live suffix in this block and stored no ranks (k_tr_sort, lazy ranks): nothing to read, nothing to count
    th[threadIdx.x] = 0;
    if (inText) tl[threadIdx.x] = 0;
    return;
  }
  const u32 subs = live_subtiles(A, b, tile, n, first);
  __shared__ u32 hist[MSD_BINS];
  __shared__ u32 subLive[4];
  hist[threadIdx.x] = 0;
  if (threadIdx.x < 4) subLive[threadIdx.x] = 0;
  __syncthreads();
  if (subs) {
    const u32* rank = A.rank + (int64_t)b * A.NS;
    const int lane = kz_lane();
    const int tbase = tile * RSORT_TILE;
    const uint64_t lt = kz_lanemask_lt();
    u32 rk[RSC_ITEMS];
#pragma unroll
    for (int r = 0; r < RSC_ITEMS; r++) {
      const int s = tbase + r * RSC_WG + (int)threadIdx.x;
      rk[r] = ((subs >> (r >> 2)) & 1u) && s < n ? rank[s] : 0u;
    }
    u32 c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < RSC_ITEMS; r++) {
      const bool live = (rk[r] & BW_LIVE) != 0;
      c[r >> 2] += (u32)__popcll(kz_ballot(live));
      (void)msd_tile_place(hist, ((rk[r] & ~BW_LIVE) >> BK_BITS) & (MSD_BINS - 1), live, lane, lt);
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) if (c[q]) atomicAdd(&subLive[q], c[q]);
    }
  }
  __syncthreads();
  th[threadIdx.x] = hist[threadIdx.x];
  if (inText) tl[threadIdx.x] = subLive[threadIdx.x];
  if (threadIdx.x == 0) {
    const u32 tot = subLive[0] + subLive[1] + subLive[2] + subLive[3];
    if (tot) atomicAdd(&A.d_m2[b], (int32_t)tot);
  }
}
__global__ __launch_bounds__(RSC_WG) void k_live_scatter(u64* __restrict__ keyOut, u32* __restrict__ valOut, BwtArrays A, int h, int bitsR) {
  const int b = bw_row_block(A, blockIdx.y);
  const int n = A.d_n[b];
  const int tile = blockIdx.x;
  if ((int64_t)tile * RSORT_TILE >= n || A.d_m[b] <= 0) return;
  const u32 subs = live_subtiles(A, b, tile, n, 0);
  if (!subs) return;                                                  // nothing left here: neither read nor written
  __shared__ u32 cnt[MSD_BINS];
  __shared__ u32 gdelta[MSD_BINS];
  __shared__ u32 scan[32];
  __shared__ u64 stage[RSORT_TILE];  // 128 KiB: keys, then values
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t off = (int64_t)b * A.NS;
  const u32* rank = A.rank + off;
  const int lane = kz_lane();
  const int tbase = tile * RSORT_TILE;
  const uint64_t lt = kz_lanemask_lt();
  const u32 hcap = (u32)min(h, n);
  u64 k[RSC_ITEMS]; u32 v[RSC_ITEMS]; u32 dr[RSC_ITEMS];
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const int s = tbase + r * RSC_WG + (int)threadIdx.x;
    v[r] = (u32)s;
    dr[r] = ((subs >> (r >> 2)) & 1u) && s < n ? rank[s] : 0u;        // the rank for now
  }
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    k[r] = 0;
    if (dr[r] & BW_LIVE) {
      const int s = tbase + r * RSC_WG + (int)threadIdx.x;
      const int64_t j = (int64_t)s + h;
      // positions past the end (s + h >= n): n - s in [1, min(h, n)], smaller for the shorter suffix and below every real rank
      const u64 r2 = (j < n) ? (u64)(rank[j] & ~BW_LIVE) + (u64)hcap + 1ULL : (u64)(n - s);
      k[r] = ((u64)(dr[r] & ~BW_LIVE) << bitsR) | r2;
    }
  }
#pragma unroll
  for (int r = 0; r < RSC_ITEMS; r++) {
    const bool live = (dr[r] & BW_LIVE) != 0;
    dr[r] = msd_tile_place(cnt, ((dr[r] & ~BW_LIVE) >> BK_BITS) & (MSD_BINS - 1), live, lane, lt);
  }
  msd_tile_flush(k, v, dr, bitsR + BK_BITS, keyOut + off, valOut + off, A, b, tile, cnt, gdelta, scan, stage);
}


// ---------------------------------------------------------------------------------------------
// emit: header + BWT bytes (BWTBlockCodec.java:90-126, DivSufSort.java:217-224)
// XCD-aware mapping: the gather s[sa[j] - 1] hits random lines of the block's text, which fits ONE XCD's L2 (4 MiB) but is evicted
// when every XCD works on every block.  Workgroup w runs on XCD w % 8 (observed dispatch order, a speed matter only), so the
// workgroups of a super-group of 8 blocks are dealt out block = w % 8: each XCD gathers from one block's text at a time.
__global__ void k_bwt_emit(const u8* __restrict__ src, int64_t srcStride, u8* __restrict__ dst, int64_t dstStride,
                           BwtArrays A, int32_t* d_lenOut, int32_t* d_flag, int B) {
  const int lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int sg = lin / (8 * (int)gridDim.x), r8 = lin % (8 * (int)gridDim.x);
  const int b = B < 0 ? (int)blockIdx.y : sg * 8 + (r8 & 7);               // B < 0: plain mapping (a grid of B rounded up to 8 rows would not fit)
  const int chunk = B < 0 ? (int)blockIdx.x : r8 >> 3;
  if (B >= 0 && b >= B) return;
  const int n = A.d_n[b];
  const u8* s = src + (int64_t)b * srcStride;
  u8* d = dst + (int64_t)b * dstStride;
  const int64_t off = (int64_t)b * A.NS;
  if (n < 2) {   // n==1: pIndexSize==0 -> BWTBlockCodec declines (BWTBlockCodec.java:95-98); n==0 no-op
    if (chunk == 0 && threadIdx.x == 0) { d_flag[b] = 0; d_lenOut[b] = n; if (n == 1) d[0] = s[0]; }
    return;
  }
  int logBlockSize = kz_ilog2((u32)n);
  if ((n & (n - 1)) != 0) logBlockSize++;
  const int pIndexSize = (logBlockSize + 7) >> 3;
  const int chunks = (n < 256) ? 1 : 8;
  const int hdr = 1 + chunks * pIndexSize;
  const u32* rank = A.rank + off;
  const u32* sa = A.sa + off;
  const int p = (int)rank[0];
  if (chunk == 0 && threadIdx.x == 0) {
    const int logNbChunks = (chunks == 8) ? 3 : 0;
    d[0] = (u8)((logNbChunks << 2) | (pIndexSize - 1));
    const int st = n / chunks;
    const int step = (st * chunks != n) ? st + 1 : st;
    int idx = 1;
    for (int k = 0; k < chunks; k++) {
      const int pi = (int)rank[(int64_t)k * step];       // primary[k]-1 = ISA[k*step]
      for (int shift = (pIndexSize - 1) << 3; shift >= 0; shift -= 8) d[idx++] = (u8)(pi >> shift);
    }
    d[hdr] = s[n - 1];
    d_lenOut[b] = hdr + n;
    d_flag[b] = 1;
  }
  for (int j = chunk * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    if (j == p) continue;
    const u32 sv = sa[j];
    const u8 c = s[sv - 1];
    d[hdr + ((j < p) ? j + 1 : j)] = c;
  }
}

// ---------------------------------------------------------------------------------------------
// host: the arena of a batch, term by term what bwt_alloc_arrays (and bwt_trie_alloc) take
size_t kz_bwt_forward_scratch(int B, int maxN) {
  const int64_t NS = (int64_t)kz_align((size_t)maxN, RS_TILE);
  const int T = (int)(NS / RS_TILE);
  size_t per = (size_t)NS * (8 * 2 + 4 * 2)      // key[2], val[2]
             + (size_t)NS * (4 + 4)              // rank, sa
             + (size_t)(T + 4) * 256 * 4         // tileHist: HS = radix tiles x MSD_BINS words, RSORT_TILE = 4 RS_TILE
             + 2 * MSD_BINS * 4                  // digitBase, bucketCnt
             + (size_t)(T + 4) * 12              // tileA, tileB, tileLive
             + 64                                // d_w, d_big, d_m, d_m2, d_act
             + 11 * 256;                         // the allocations' alignment
  if (tr_applies(maxN)) per += bwt_trie_scratch(maxN);
  return kz_align(per * (size_t)B + 4096 * 16, 4096) + (1 << 20);
}
static bool bwt_alloc_arrays(BwtRun& R) {
  BwtArrays& A = R.A;
  const size_t B = (size_t)R.B, NS = (size_t)R.NS, T = (size_t)R.T;
  bool ok = true;
  auto take = [&](size_t bytes) { void* p = kz_arena_alloc(R.ctx, bytes); ok = ok && p != nullptr; return p; };
  for (int i = 0; i < 2; i++) { A.key[i] = (u64*)take(NS * B * 8); A.val[i] = (u32*)take(NS * B * 4); }
  A.rank = (u32*)take(NS * B * 4);
  A.sa = (u32*)take(NS * B * 4);
  A.tileHist = (u32*)take((size_t)A.HS * B * 4);
  A.digitBase = (u32*)take(B * MSD_BINS * 4);
  A.bucketCnt = (u32*)take(B * MSD_BINS * 4);
  A.d_w = (int32_t*)take(B * 4);
  A.d_big = (int32_t*)take(B * 4);
  A.tileA = (u32*)take(T * B * 4);
  A.tileB = (u32*)take(T * B * 4);
  A.tileLive = (u32*)take(T * B * 4);
  A.d_m = (int32_t*)take(B * 4);
  A.d_m2 = (int32_t*)take(B * 4);
  R.d_act = (int32_t*)take(B * 4);
  return ok;
}

static const int BW_K0 = 7;                                        // bytes of the first-round key
static const int BW_BUCKET_MIN = 4096;                             // below: the whole list is a handful of LSD tiles

// geometry, switches and arrays of one pass over the batch
static int bwt_plan(BwtRun& R, kz_ctx* ctx, kz_batch& bt, bool allowTrie) {
  R.ctx = ctx; R.bt = &bt; R.B = bt.B;
  for (int b = 0; b < bt.B; b++) if (bt.h_len[b] > R.maxN) R.maxN = bt.h_len[b];
  const int maxN = R.maxN;
  R.NS = (int64_t)kz_align((size_t)(maxN > 0 ? maxN : 1), RS_TILE);
  R.T = (int)(R.NS / RS_TILE);
  R.A.NS = R.NS; R.A.T = R.T; R.A.HS = (int64_t)((R.NS + RSORT_TILE - 1) / RSORT_TILE) * MSD_BINS;
  if (!bwt_alloc_arrays(R)) { snprintf(ctx->err, sizeof(ctx->err), "bwt_forward: arena overflow"); return -KZ_ERR_DEVICE; }
  // the caller sized the arena for the longest block the CHAIN can hand over, which may lie outside the trie rounds' range while
  // this batch's blocks are inside: the LSD rounds need no tables
  R.useTrie = allowTrie && ctx->sw.bwtTrie != 0 && tr_applies(maxN) && bwt_trie_alloc(ctx, bt.B, maxN, R.TR);
  R.A.d_n = bt.d_len;
  R.bitsR = 1;
  while ((1LL << R.bitsR) < 2 * (int64_t)maxN + 2) R.bitsR++;       // secondary key < n + h + 1 <= 2n + 1
  R.bitsG = 1;
  while ((1LL << R.bitsG) < (int64_t)maxN) R.bitsG++;
  // bucket path of the later rounds: the packed LDS element needs BK_BITS + bitsR + bitsG <= 64
  R.nBuckets = 1 << (R.bitsG > BK_BITS ? R.bitsG - BK_BITS : 0);
  R.useBuckets = (BK_BITS + R.bitsR + R.bitsG <= 64) && R.nBuckets <= MSD_BINS && ctx->sw.bwtBuckets != 0;
  R.Dmax = (ctx->sw.bwtDmax >= 6 && ctx->sw.bwtDmax <= TR_DMAX_LIMIT) ? ctx->sw.bwtDmax : 6;
  R.noRetire = ctx->sw.bwtRetire == 0;                              // A/B switch: every block rides through every round, as before
  R.trieWinOff = ctx->sw.bwtTrieWin == 0;
  R.lazyRank = ctx->sw.bwtLazyRank != 0;
  R.livePart = ctx->sw.bwtLivePart < 0 ? 1 : ctx->sw.bwtLivePart;   // A/B switch: 0 = every later round from the text-order list, as before
  R.trace = ctx->sw.bwtTrace != 0;
  R.forceOvfRound = ctx->sw.bwtTestTrieOverflow;                    // tests: pretend the tables overflowed in round <digit>
  R.kC = R.A.key[0]; R.kF = R.A.key[1]; R.vC = R.A.val[0]; R.vF = R.A.val[1];
  R.nAct = bt.B;
  R.h_act = ctx->hpin + bt.B + 16;                                  // (pipe_setup reserves 9 B + 64 ints)
  R.mMax = maxN;
  return 0;
}

// the bucket partition of the live suffixes into (kF, vF): from the ranks (k_live_hist counted at the end of the round before), or
// from the text-order list in (kC, vC)
static int bwt_partition(BwtRun& R) {
  kz_ctx* ctx = R.ctx; BwtArrays& A = R.A;
  const int nAct = R.nAct;
  const int rt = gridFor(R.fromRanks ? R.maxN : R.mMax, RSORT_TILE);
  const int sh = R.bitsR + BK_BITS;
  if (!R.fromRanks) KZ_LAUNCH(ctx, KID_MSD_HIST, k_msd_hist, dim3(rt, nAct), dim3(KZ_WG), R.kC, A, sh);
  KZ_LAUNCH(ctx, KID_MSD_SCAN, k_msd_scan, dim3(nAct), dim3(MSD_BINS), A, R.fromRanks ? 1 : 0);
  KZ_HIP(hipMemcpyAsync(ctx->hpin, A.d_big, (size_t)R.B * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (R.fromRanks) KZ_LAUNCH(ctx, KID_MSD_SCATTER, k_live_scatter, dim3(rt, nAct), dim3(RSC_WG), R.kF, R.vF, A, R.h, R.bitsR);
  else KZ_LAUNCH(ctx, KID_MSD_SCATTER, k_msd_scatter, dim3(rt, nAct), dim3(RSC_WG), R.kC, R.vC, R.kF, R.vF, A, sh);
  return 0;
}

// a later round of blocks up to 4 MiB: bucket partition + one LDS kernel per bucket; what is left for the window comes back in wMax
static int bwt_round_buckets(BwtRun& R, int round) {
  kz_ctx* ctx = R.ctx; BwtArrays& A = R.A;
  const int nAct = R.nAct, nBuckets = R.nBuckets;
  const int rc = bwt_partition(R);
  if (rc) return rc;
  R.swap();
  KZ_LAUNCH(ctx, KID_BUCKET_COUNT_S, k_bucket_count_s, dim3(nBuckets, nAct), dim3(256), R.kC, R.vC, A, R.bitsR, R.bitsG, (u32)BK_GMAX);
  KZ_LAUNCH(ctx, KID_BUCKET_COUNT, k_bucket_count, dim3(nBuckets, nAct), dim3(1024), R.kC, R.vC, A, R.bitsR, R.bitsG, (u32)BK_GMAX);
  KZ_LAUNCH(ctx, KID_BUCKET_SORT, k_bucket_sort, dim3(nBuckets, nAct), dim3(1024), R.kC, R.vC, A, R.bitsR, R.bitsG);
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  R.wMax = 0;                                                      // (a retired block's d_big is stale: only the live rows count)
  long long tot = 0;
  for (int r = 0; r < nAct; r++) { const int w = ctx->hpin[A.act ? R.h_act[r] : r]; tot += w; if (w > R.wMax) R.wMax = w; }
  R.windowed = true;
  if (R.trace) fprintf(stderr, "[bwt] round %d: %lld suffixes in oversized buckets, max per block %d\n", round, tot, R.wMax);
  return 0;
}

// LSD radix over the window [d_w, d_m) of the compact list (the whole list without buckets), then SA order: new groups, ranks, final suffixes
static int bwt_round_lsd(BwtRun& R, int round) {
  kz_ctx* ctx = R.ctx; const BwtArrays& A = R.A;
  const int nAct = R.nAct;
  const int nbits = (round == 0) ? 8 * BW_K0 : R.bitsR + R.bitsG;
  const int passes = (nbits + 7) / 8;
  const int gshift = (round == 0) ? 64 : R.bitsR;
  const int tiles = gridFor(R.wMax, RS_TILE);
  const int rtiles = gridFor(R.wMax, RSORT_TILE);
  for (int p = 0; p < passes; p++) {
    if (round == 0 && p == 0) {                                    // keys straight from the text
      const TextSrc X0 = {R.bt->buf[R.bt->cur], R.bt->stride, BW_K0};
      KZ_LAUNCH(ctx, KID_RADIX_HIST, k_radix_hist0, dim3(rtiles, nAct), dim3(KZ_WG), A, X0);
      KZ_LAUNCH(ctx, KID_RADIX_SCAN, k_radix_scan, dim3(nAct), dim3(256), A);
      KZ_LAUNCH(ctx, KID_RADIX_SCATTER, k_radix_scatter0, dim3(rtiles, nAct), dim3(RSC_WG), R.kF, R.vF, A, X0);
    } else {
      KZ_LAUNCH(ctx, KID_RADIX_HIST, k_radix_hist, dim3(rtiles, nAct), dim3(KZ_WG), R.kC, A, p * 8);
      KZ_LAUNCH(ctx, KID_RADIX_SCAN, k_radix_scan, dim3(nAct), dim3(256), A);
      KZ_LAUNCH(ctx, KID_RADIX_SCATTER, k_radix_scatter, dim3(rtiles, nAct), dim3(RSC_WG), R.kC, R.vC, R.kF, R.vF, A, p * 8);
    }
    R.swap();
  }
  KZ_LAUNCH(ctx, KID_SEG_REDUCE, k_seg_reduce, dim3(tiles, nAct), dim3(KZ_WG), R.kC, A, gshift);
  KZ_LAUNCH(ctx, KID_SEG_SCAN, k_seg_scan, dim3(nAct), dim3(64), A);
  KZ_LAUNCH(ctx, KID_SEG_APPLY, k_seg_apply, dim3(tiles, nAct), dim3(KZ_WG), R.kC, R.vC, A, gshift);
  return 0;
}

// text order: the live suffixes with their keys as a compact list in (kC, vC), for the rounds that sort the whole list
static int bwt_live_list(BwtRun& R, bool first) {
  kz_ctx* ctx = R.ctx; BwtArrays& A = R.A;
  KZ_HIP(hipMemsetAsync(A.d_m2, 0, (size_t)R.B * 4, ctx->stream));
  KZ_LAUNCH(ctx, KID_LIVE_EMIT, k_live_emit, dim3(gridFor(R.maxN, RS_TILE), R.nAct), dim3(KZ_WG), R.kF, R.vF, A, R.h, R.bitsR, first ? 1 : 0,
            (first && R.useTrie && R.lazyRank) ? R.TR.meta : (const int32_t*)nullptr);
  R.swap();
  return 0;
}
// ... or only their number per bucket and sort tile of the text: a bucket round takes them from the ranks (k_live_scatter)
static int bwt_live_count(BwtRun& R, bool first) {
  kz_ctx* ctx = R.ctx; BwtArrays& A = R.A;
  KZ_HIP(hipMemsetAsync(A.d_m2, 0, (size_t)R.B * 4, ctx->stream));
  KZ_LAUNCH(ctx, KID_MSD_HIST, k_live_hist, dim3(gridFor(R.maxN, RSORT_TILE), R.nAct), dim3(RSC_WG), A, first ? 1 : 0,
            (first && R.useTrie && R.lazyRank) ? R.TR.meta : (const int32_t*)nullptr);
  return 0;
}
// does the next round partition straight from the ranks?  (livePart = N >= 2: only while the longest list is above maxN / N)
static bool bwt_next_from_ranks(const BwtRun& R) {
  if (!R.livePart || !R.useBuckets || R.mMax < BW_BUCKET_MIN) return false;
  return R.livePart < 2 || (int64_t)R.mMax * R.livePart >= (int64_t)R.maxN;
}

// count or compact the live suffixes for the next round, and read the next compact sizes back
static int bwt_compact_and_read_back(BwtRun& R, int round, bool* trieOverflow) {
  kz_ctx* ctx = R.ctx; BwtArrays& A = R.A;
  const int B = R.B;
  hipStream_t st = ctx->stream;
  R.h = (round == 0) ? (R.useTrie ? 6 : BW_K0) : R.h * 2;
  const bool count = R.livePart && R.useBuckets;                  // the list is written once the sizes say that the next round needs it
  int rc = count ? bwt_live_count(R, round == 0) : bwt_live_list(R, round == 0);
  if (rc) return rc;
  KZ_HIP(hipMemcpyAsync(ctx->hpin, A.d_m2, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  // the trie tables' overflow flag rides along, every round that ran a trie (round 0 and the key rounds of the window): an
  // overflow dropped buckets, the ranks of this pass are void (the bounds of tr_max_nodes / tr_max_buckets say it cannot happen)
  ctx->hpin[B] = 0;
  if (R.useTrie) KZ_HIP(hipMemcpyAsync(ctx->hpin + B, R.TR.err, 4, hipMemcpyDeviceToHost, st));
  KZ_HIP(kz_stream_sync(ctx, st));
  R.mMax = 0;
  for (int b = 0; b < B; b++) if (ctx->hpin[b] > R.mMax) R.mMax = ctx->hpin[b];
  if (R.useTrie && (ctx->hpin[B] != 0 || round == R.forceOvfRound)) { *trieOverflow = true; return 0; }
  if (R.trace) {                                   // diagnostic: live suffixes left after every doubling round
    long long tot = 0, totN = 0; for (int b = 0; b < B; b++) { tot += ctx->hpin[b]; totN += R.bt->h_len[b]; }
    fprintf(stderr, "[bwt] round %d h=%d: live %lld of %lld (%.1f%%), max per block %d\n", round, R.h, tot, totN, 100.0 * tot / (totN ? totN : 1), R.mMax);
  }
  std::swap(A.d_m, A.d_m2);
  R.fromRanks = bwt_next_from_ranks(R);
  if (count && !R.fromRanks && R.mMax > 0) rc = bwt_live_list(R, false);      // (tileLive is k_live_hist's: no tile is `first`)
  return rc;
}

// retire the blocks that are done: the next round's grids get one row per block that still has live suffixes
static int bwt_retire(BwtRun& R) {
  kz_ctx* ctx = R.ctx;
  if (R.mMax <= 0 || R.noRetire) return 0;
  int cnt = 0;
  for (int b = 0; b < R.B; b++) if (ctx->hpin[b] > 0) R.h_act[cnt++] = b;     // (hpin[0 .. B) is read before the next copy lands: in-order stream)
  if (cnt < R.B) {
    KZ_HIP(hipMemcpyAsync(R.d_act, R.h_act, (size_t)cnt * 4, hipMemcpyHostToDevice, ctx->stream));
    R.A.act = R.d_act;
    R.nAct = cnt;
  }
  return 0;
}

static int bwt_emit(BwtRun& R) {
  kz_ctx* ctx = R.ctx; kz_batch& bt = *R.bt;
  const int B = R.B;
  const int rows8 = (B + 7) / 8 * 8;
  const bool xcd = rows8 <= KZ_MAX_BATCH;
  KZ_LAUNCH(ctx, KID_BWT_EMIT, k_bwt_emit, dim3(gridFor(R.maxN, 256 * 8), xcd ? rows8 : B), dim3(256), bt.buf[bt.cur], bt.stride, bt.buf[bt.cur ^ 1], bt.stride,
            R.A, bt.d_len2, bt.d_flag, xcd ? B : -1);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  std::swap(bt.d_len, bt.d_len2);
  return 0;
}

// one pass of the stage; *trieOverflow is set (and nothing of the batch changed) when a trie table overflowed in any round.
// A round sorts (kC, vC) and applies the new groups by ONE of four paths -- the trie round over the text (round 0), else the bucket
// partition with the window of oversized buckets through a key trie round or through the LSD passes, else the LSD passes over the
// whole compact list -- and then compacts what is still live.
static int bwt_forward_run(kz_ctx* ctx, kz_batch& bt, bool allowTrie, bool* trieOverflow) {
  BwtRun R{};
  int rc = bwt_plan(R, ctx, bt, allowTrie);
  if (rc) return rc;
  KZ_LAUNCH(ctx, KID_BWT_INIT, k_bwt_init, dim3((R.B + 255) / 256), dim3(256), R.A, R.B);
  if (R.useTrie) KZ_HIP(hipMemsetAsync(R.TR.err, 0, 4, ctx->stream));
  for (int round = 0; round < 64 && R.mMax > 0; round++) {
    const bool buckets = R.useBuckets && round > 0 && R.mMax >= BW_BUCKET_MIN;
    R.wMax = R.mMax;
    if (round == 0 && R.useTrie) { rc = bwt_trie_text_round(R); R.wMax = 0; }
    else if (buckets) rc = bwt_round_buckets(R, round);
    else if (R.windowed) { KZ_HIP(hipMemsetAsync(R.A.d_w, 0, (size_t)R.B * 4, ctx->stream)); R.windowed = false; }
    if (rc) return rc;
    const bool trieWindow = R.useTrie && buckets && R.wMax > 0 && R.bitsR <= 24 && R.bitsG <= 24 && !R.trieWinOff;
    if (trieWindow) rc = bwt_trie_key_round(R);
    else if (R.wMax > 0) rc = bwt_round_lsd(R, round);
    if (rc) return rc;
    rc = bwt_compact_and_read_back(R, round, trieOverflow);
    if (rc || *trieOverflow) return rc;
    if ((rc = bwt_retire(R)) != 0) return rc;
  }
  if (R.mMax > 0) { snprintf(ctx->err, sizeof(ctx->err), "bwt_forward: suffix sort did not converge"); return -KZ_ERR_PROCESS_BLOCK; }
  return bwt_emit(R);
}

int kz_stage_bwt_forward(kz_ctx* ctx, kz_batch& bt) {
  const size_t mark = ctx->arenaTop;
  bool overflow = false;
  int rc = bwt_forward_run(ctx, bt, true, &overflow);
  if (rc == 0 && overflow) {                                       // redo the batch on the LSD rounds (no tables to overflow); the input buffer is untouched
    ctx->arenaTop = mark;
    overflow = false;
    rc = bwt_forward_run(ctx, bt, false, &overflow);
  }
  return rc;
}
