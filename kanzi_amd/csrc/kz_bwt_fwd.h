// kz_bwt_fwd.h -- what the two translation units of the forward BWT share: kz_bwt_fwd.hip (radix / bucket rounds, emit, the driver)
// and kz_bwt_trie.hip (the trie round over the text and over a doubling round's window).  The arrays, the constants, and the device
// mechanisms that more than one kernel uses, each of them ONCE: a kernel body calls the helper, it does not copy it (the one exception,
// the pass loop of the LDS sorts, is explained at bucket_body).  All helpers are __device__ __forceinline__; the __shared__ arrays
// stay declared in the kernel bodies and are passed in.
#pragma once
#include "kz_device.h"
#include "kz_internal.h"
#include <utility>

#define BW_LIVE 0x80000000u

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint8_t u8;
typedef u64 __attribute__((aligned(1))) bw_u64_unaligned;

struct BwtArrays {
  u64* key[2]; u32* val[2];
  u32* rank; u32* sa;
  u32* tileHist;     // [B][radix tiles][256 | MSD_BINS]
  u32* digitBase;    // [B][MSD_BINS]
  u32* bucketCnt;    // [B][MSD_BINS] elements per bucket of the current round (bit 31: too large for the LDS sort)
  int32_t* d_w;      // [B] window start: the LSD passes and the k_seg_* kernels work on [d_w, d_m) of the compact arrays
  int32_t* d_big;    // [B] d_m - d_w after k_msd_scan
  u32* tileA;        // [B][T] scan temporaries
  u32* tileB;        // [B][T]
  u32* tileLive;     // [B][T] live suffixes of the text tile in the previous round (0 stays 0: suffixes only become final)
  int32_t* d_n;      // [B] block length
  int32_t* d_m;      // [B] compact size (current)
  int32_t* d_m2;     // [B] compact size (next)
  int64_t NS;        // element stride per block
  int T;             // tile stride per block
  int64_t HS;        // tileHist stride per block: radix tiles x MSD_BINS
  const int32_t* act; // later rounds: the blocks that still have live suffixes, one grid row each (nullptr: row = block)
};
// A block whose suffixes are all final takes no part in the later rounds: their grids have one row per block that is still live
// (a mixed batch used to carry the uniform / geometric blocks' empty workgroups through every round).
__device__ __forceinline__ int bw_row_block(const BwtArrays& A, unsigned row) { return A.act ? A.act[row] : (int)row; }

// lanes of the wave whose NBITS-bit digit equals this lane's (0 for a lane that is not valid).
// Per digit bit: x = the lane's bit spread over a word (0 / ~0), bal = the lanes whose bit is set; the lanes that agree with this lane
// in the bit are ~(bal ^ x).  Kept in 32-bit halves: the compiler then spends six VALU instructions per bit (shift, v_bfe_i32, v_cmp,
// two v_xor and half a v_or3 over the differences) instead of the nine of `m &= bit ? bal : ~bal` on 64-bit masks; the ranking phase of
// the LDS sorts is VALU bound (k_tr_sort 39.8 -> 36.8 ms, k_bucket_sort 16.9 -> 15.3 ms per 342 mixed blocks).  A hand-scheduled
// four-instruction form (v_bfe_i32, v_cmp into an SGPR pair, two v_bitop3_b32 reading it) is correct but SLOWER (50.7 ms): an
// instruction with an SGPR operand occupies the SIMD twice as long as a VGPR-only one (tools/ubench_valu_rate.hip) and a VALU read of an
// SGPR that a VALU compare just wrote stalls the wave for about 16 cycles.
template <int NBITS>
__device__ __forceinline__ uint64_t bw_match(u32 d, bool valid) {
  const uint64_t m0 = kz_ballot(valid);
  u32 mlo = (u32)m0, mhi = (u32)(m0 >> 32);
#pragma unroll
  for (int b = 0; b < NBITS; b++) {
    const u32 x = (u32)(((int32_t)(d << (31 - b))) >> 31);
    const uint64_t bal = kz_ballot(x != 0u);
    mlo &= ~((u32)bal ^ x);
    mhi &= ~((u32)(bal >> 32) ^ x);
  }
  return valid ? (((uint64_t)mhi << 32) | mlo) : 0ULL;
}

// ---------------------------------------------------------------------------------------------
// The buckets of a later round (k_msd_* partition, k_bucket_count*, k_bucket_sort: see kz_bwt_fwd.hip)
#define BK_BITS 12
#define BK_CAP 6144            // 4096 slots + an overhang of 2048: 48 KiB of LDS, two workgroups per CU
#define BK_BIG 0x80000000u
#define BK_DBITS 9             // LDS sort digit: 36 key bits of a 4 MiB block in four passes
#define BK_DBINS (1 << BK_DBITS)
#define BK_SMALL 1024
#define BK_SORT 0x40000000u
#define BK_GMAX 256
#define BK_SLOTS (1 << BK_BITS)

// ---------------------------------------------------------------------------------------------
// The trie rounds (kz_bwt_trie.hip)
#define TR_META 32               // ints per block: [0] nodes, [1] buckets, [2 + L] first node of depth L, [10 + L] end, [18] error, [20] lazy ranks: live suffixes found
#define TR_CAP 7680u             // LDS sort capacity (60 KiB of elements + 16 KiB of counters: two workgroups per CU)
#define TR_MERGE (TR_CAP / 2)    // siblings above this are a bucket of their own
#define TR_K_SMALL 1u
#define TR_K_EXP 2u
#define TR_K_TERM 3u
#define TR_UNCHANGED (1u << 29)     // key rounds, terminal child: the new group keeps the old group's head slot (its members' ranks stay)
#define TR_NODECHUNK 128         // nodes whose counters fit the LDS of k_tr_count
#define TR_MAXB 12288
#define TR_DMAX_LIMIT 7
#define TR_MIN_N 65536
#define TR_MAX_N ((4 << 20) + 65536)
// move every suffix once: tile = 8192 suffixes in text order.  The tile's count per bucket lives in 16-bit halves of LDS words (a
// tile holds at most 8192 suffixes), so that TR_MAXB buckets fit next to the staging buffer.
#define TRS_TILE 8192
// Two sizes of the same kernel (round 5): blocks with at most TRS_FASTB buckets (every block measured: 456 .. 790) take tiles of 4096
// suffixes with 52 KiB of LDS -- three workgroups per CU to hide the state -> info -> text chain -- the others the full tables
// (152 KiB, one workgroup per CU).  Both are launched; a block's workgroups of the form that is not its own return at once.
#define TRS_FASTB 2048
#define TRQ_WAVES 16             // the bucket sort's workgroup: 16 waves x up to 8 rows of 64 elements
#define TRQ_ROWS 8
struct TrieArrays {
  u32* cnt;        // [B][MN][256] children counts
  u32* info;       // [B][MN][256] kind << 30 | payload (SMALL: skip << 16 | bucket; EXP: node; TERM: head slot)
  u32* nodeStart;  // [B][MN] first slot of the node's range
  u32* bStart;     // [B][MB]
  u32* bCount;     // [B][MB]
  u32* bFill;      // [B][MB] elements placed so far (k_tr_scatter)
  u32* bAux;       // [B][MB] key rounds: skip >= 3: slot of the bucket's first element (g + bStart - group start); skip < 3: the bucket's prefix bytes
  u32* bG;         // [B][MB] key rounds, skip >= 3: the old group g all elements of the bucket belong to
  u32* nodePfx;    // [B][MN] key rounds: the node's prefix bytes (depth < 3) or its old group g (depth >= 3)
  u32* nodeGS;     // [B][MN] key rounds, depth >= 3: position of the old group's first element in the sorted window
  int32_t* meta;   // [B][TR_META]
  int32_t* err;    // [1] set when a table overflows (cannot happen for blocks the host admits: see tr_max_nodes / tr_max_buckets)
  int MN, MB;
};
// one block's tables
struct TrieView { u32 *cnt, *info, *nodeStart, *bStart, *bCount, *bFill, *bAux, *bG, *nodePfx, *nodeGS; int32_t* meta; };
__device__ __forceinline__ TrieView tr_view(const TrieArrays& T, int b) {
  const int64_t n = (int64_t)b * T.MN, k = (int64_t)b * T.MB;
  return TrieView{T.cnt + n * 256, T.info + n * 256, T.nodeStart + n, T.bStart + k, T.bCount + k, T.bFill + k, T.bAux + k, T.bG + k,
                  T.nodePfx + n, T.nodeGS + n, T.meta + (int64_t)b * TR_META};
}

__device__ __forceinline__ u32 tr_byte(const u8* __restrict__ s, int i, int n) { return i < n ? (u32)s[i] : 0u; }

// 32768 LDS words: the byte-pair half table of k_[trk_]hist16 and the counters of a node chunk of k_[trk_]count
static_assert(TR_NODECHUNK * 256 == 32768, "one LDS table size for the histogram and the count kernels");
__device__ __forceinline__ void trc_zero_chunk(u32* lds) {
  for (int i = threadIdx.x; i < TR_NODECHUNK * 256; i += 1024) lds[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void tr_hist16_flush(const u32* hist, u32* __restrict__ out) {
  __syncthreads();
  for (int i = threadIdx.x; i < 32768; i += 1024) out[i] = hist[i];
}
// k_[trk_]count, one quad of consecutive items (the first `left` of them exist): apply the looked-up info entries to the states that
// asked for one (look), find each item's counter among the chunk's nodes [nlo, nlo + TR_NODECHUNK) by its byte cb, and add to LDS
// once per run of equal targets.  Returns whether a state changed (the caller stores the quad).
__device__ __forceinline__ bool trc_resolve_quad(u32 (&stq)[4], const u32 (&e)[4], const bool (&look)[4], const u32 (&cb)[4],
                                                 int left, int L, int nlo, u32* lds) {
  bool changed = false;
  u32 runT = 0xFFFFFFFFu, runC = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    u32 tgt = 0xFFFFFFFFu;
    if (q < left && (stq[q] >> 30) == 0) {
      if (look[q]) {
        stq[q] = ((e[q] >> 30) == TR_K_EXP) ? ((e[q] & 0xFFFFu) | ((u32)L << 16)) : e[q];
        changed = true;
      }
      if ((stq[q] >> 30) == 0) {                                           // inside a node of depth L now
        const int k = (int)(stq[q] & 0xFFFFu) - nlo;
        if (k >= 0 && k < TR_NODECHUNK) tgt = (u32)k * 256 + cb[q];
      }
    }
    if (tgt == runT) runC++;
    else {
      if (runC && runT != 0xFFFFFFFFu) atomicAdd(&lds[runT], runC);
      runT = tgt; runC = 1;
    }
  }
  if (runC && runT != 0xFFFFFFFFu) atomicAdd(&lds[runT], runC);
  return changed;
}
__device__ __forceinline__ void trc_flush_chunk(const u32* lds, u32* __restrict__ cnt, int nlo, int hi) {
  __syncthreads();
  for (int j = threadIdx.x; j < TR_NODECHUNK * 256; j += 1024) {
    const u32 v = lds[j];
    if (v && nlo + (j >> 8) < hi) atomicAdd(&cnt[(int64_t)(nlo + (j >> 8)) * 256 + (j & 255)], v);
  }
  __syncthreads();
}

// k_[trk_]scatter: an element of bucket bk takes the next position of its (tile, bucket) counter; returns bucket | position << 16
__device__ __forceinline__ u32 tr_tile_place(u32* tc2, u32 bk) {
  const u32 old = atomicAdd(&tc2[bk >> 1], (bk & 1u) ? 65536u : 1u);
  return bk | (((bk & 1u) ? (old >> 16) : (old & 0xFFFFu)) << 16);
}
// ... and the tile leaves: exclusive scan of the tile's bucket counts (a thread owns whole words), buckets present reserve their run
// in the bucket's slot range (bFill), the elements are staged in bucket order and written out in runs.  bp[r] = 0xFFFFFFFF: no element.
template <int TILE_>
__device__ __forceinline__ void tr_tile_flush(const u64 (&el)[TILE_ / 1024], const u32 (&bp)[TILE_ / 1024], int nB, const TrieView& V,
                                              u64* __restrict__ elem, u32* tc2, u32* gdelta, u64* stage, uint16_t* stageB, u32* scan) {
  __syncthreads();
  {
    const int per = 2 * ((nB + 2047) / 2048);
    const int j0 = threadIdx.x * per;
    u32 mine = 0;
    for (int j = j0; j < j0 + per && j < nB; j += 2) { const u32 w = tc2[j >> 1]; mine += (w & 0xFFFFu) + (w >> 16); }
    u32 total;
    u32 run = kz_wg_excl_sum(mine, scan, &total);
    for (int j = j0; j < j0 + per && j < nB; j += 2) {
      const u32 w = tc2[j >> 1];
      const u32 c0 = w & 0xFFFFu, c1 = w >> 16;
      if (c0) gdelta[j] = V.bStart[j] + atomicAdd(&V.bFill[j], c0) - run;
      const u32 r1 = run + c0;
      if (c1) gdelta[j + 1] = V.bStart[j + 1] + atomicAdd(&V.bFill[j + 1], c1) - r1;
      tc2[j >> 1] = run | (r1 << 16);                                    // tile-local start of both buckets (< 8192 unless the bucket is empty)
      run = r1 + c1;
    }
    if (threadIdx.x == 0) scan[31] = total;
  }
  __syncthreads();
  const u32 total = scan[31];
#pragma unroll
  for (int r = 0; r < TILE_ / 1024; r++) {
    if (bp[r] != 0xFFFFFFFFu) {
      const u32 bk = bp[r] & 0xFFFFu;
      const u32 w = tc2[bk >> 1];
      const u32 slot = ((bk & 1u) ? (w >> 16) : (w & 0xFFFFu)) + (bp[r] >> 16);
      stage[slot] = el[r]; stageB[slot] = (uint16_t)bk;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < TILE_ / 1024; r++) {
    const u32 slot = (u32)r * 1024 + threadIdx.x;
    if (slot < total) elem[gdelta[stageB[slot]] + slot] = stage[slot];
  }
}

// ---------------------------------------------------------------------------------------------
// host: one pass of the stage over a batch.  bwt_plan fills it, the steps of the driver (kz_bwt_fwd.hip) and the two trie rounds
// (kz_bwt_trie.hip: a kernel is launched from the translation unit that defines it) take it.
struct BwtRun {
  kz_ctx* ctx; kz_batch* bt;
  BwtArrays A; TrieArrays TR;
  int B, maxN, T; int64_t NS;
  int bitsR, bitsG, nBuckets, Dmax;
  bool useBuckets, useTrie;
  bool noRetire, trieWinOff, lazyRank, trace; int forceOvfRound;      // the context's switches (kz_switches: read when the context was created)
  int livePart; bool fromRanks;                                        // KZ_BWT_LIVEPART; this round's bucket partition reads the ranks (k_live_hist counted)
  u64 *kC, *kF; u32 *vC, *vF;                                          // the compact pairs: current / free
  void swap() { std::swap(kC, kF); std::swap(vC, vF); }
  int nAct;                                                            // grid rows of the later rounds: blocks with live suffixes (A.act)
  int32_t *h_act, *d_act;                                              // their indices, host and device side
  int mMax, wMax;                                                      // largest compact list / largest LSD window of the batch
  int h; bool windowed;
};
static inline int gridFor(int n, int per) { int g = (n + per - 1) / per; return g < 1 ? 1 : g; }

bool tr_applies(int maxN);
size_t bwt_trie_scratch(int maxN);                                     // bytes per block of what bwt_trie_alloc takes
bool bwt_trie_alloc(kz_ctx* ctx, int B, int maxN, TrieArrays& TR);     // false: the arena is too small (and is left as it was)
int bwt_trie_text_round(BwtRun& R);                                    // round 0: the text, elements in key[0], states in val[0]
int bwt_trie_key_round(BwtRun& R);                                     // a later round's window [d_w, d_m) of (kC, vC), through (kF, vF)
