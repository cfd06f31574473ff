// kz_bwt_trie.hip -- the trie round of the forward BWT (see kz_bwt_fwd.hip for the suffix sort it is a part of), in both forms:
// over the text (round 0, k_tr_*) and over the window of a doubling round (k_trk_*), their tables, and the two host steps that
// launch them.  The constants, the tables and the device code both forms share are in kz_bwt_fwd.h.
#include "kz_bwt_fwd.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------
// Round 0 as a TRIE round: count first, move once.
// The seven LSD passes of the old round 0 moved every suffix seven times (24 B per pass) to learn, for three of
// the five data classes, that half of the suffixes sit in groups of many thousand equal 7-byte prefixes which no
// amount of sorting can split.  Here the text is only COUNTED, level by level, until every prefix class is either
// small enough to be finished in LDS or known to be one large group:
//   node   = a prefix of d bytes shared by more than TR_CAP suffixes (depth-1 nodes = the 256 first bytes, always
//            expanded); its 256 children are counted by the next byte (k_tr_hist16 for depth 1: LDS histogram of byte
//            pairs; k_tr_count for the deeper levels: LDS counters of the level's nodes, one info lookup per suffix);
//   k_tr_assign turns the counts of a level into child ranges of the suffix array (slots) and classifies each child:
//            EXPANDED (count > TR_CAP and depth < Dmax: a node of the next level), TERMINAL (count > TR_CAP at depth
//            Dmax: one group, nothing to sort), or SMALL: consecutive small siblings are merged greedily into buckets
//            of at most TR_CAP suffixes (a bucket is a contiguous slot range);
//   k_tr_scatter moves every suffix ONCE: terminal ones just get their group's head slot as rank (a coalesced store in
//            text order, they are never moved at all); the others go to their bucket as one 8-byte element
//            (the 64 - bitsG key bits that follow the bucket's common prefix | suffix index), staged per tile in LDS
//            so that a bucket's elements leave in runs;
//   k_tr_sort sorts one bucket in LDS (LSD radix over the bits that differ inside the bucket only), finds the groups
//            of equal keys and writes ranks and final suffixes like k_seg_apply.
// Depth: a bucket whose common prefix has d >= 1 bytes is sorted to d + (64 - bitsG) / 8 >= 6 bytes (zero padded at the
// end of the text like the old keys), terminal groups share Dmax >= 6 bytes.  The ranks are therefore a refinement of
// the 6-byte order and a coarsening of the suffix order, which is all the doubling rounds (h = 6, 12, ...) need: equal
// rank => equal 6-byte prefix; different rank => the true order.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the trie rounds are sized for gfx950's 160 KiB of LDS per workgroup (k_tr_hist16 128 KiB, k_tr_scatter / k_trk_scatter 152 KiB, the bucket sorts 77 KiB)"
#endif
// level 1: histogram of byte pairs (x[i], x[i+1]), x[n] = 0, one half of the 65536 bins per workgroup
__global__ __launch_bounds__(1024) void k_tr_hist16(const u8* __restrict__ srcAll, int64_t stride, BwtArrays A, TrieArrays T) {
  const int b = blockIdx.y;
  const int n = A.d_n[b];
  const u32 half = blockIdx.x;
  __shared__ u32 hist[32768];
  trc_zero_chunk(hist);
  const u8* s = srcAll + (int64_t)b * stride;
  const int lane = kz_lane();
  for (int base = 0; base < n; base += 1024 * 16) {
    const int p = base + threadIdx.x * 16;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (p < n) q = *(const uint4*)(s + p);                               // blocks are 256-byte aligned with >= 4 KiB of slack
    u32 nxt = (u32)__shfl_down((int)(q.x & 0xFFu), 1, 64);
    if (lane == 63) nxt = (p + 16 < n) ? (u32)s[p + 16] : 0u;
    const u32 w[5] = {q.x, q.y, q.z, q.w, nxt};
    u32 runKey = 0xFFFFFFFFu, runCnt = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int i = p + j;
      const u32 c0 = (w[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
      const u32 c1r = (w[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xFFu;
      const u32 c1 = (i + 1 < n) ? c1r : 0u;
      const u32 key = (c0 << 8) | c1;
      const bool mine = i < n && (key >> 15) == half;
      if (mine && key == runKey) runCnt++;
      else {
        if (runCnt) atomicAdd(&hist[runKey & 32767u], runCnt);
        runKey = mine ? key : 0xFFFFFFFFu; runCnt = mine ? 1u : 0u;
      }
    }
    if (runCnt) atomicAdd(&hist[runKey & 32767u], runCnt);
  }
  tr_hist16_flush(hist, tr_view(T, b).cnt + half * 32768);
}

// classify the children of the nodes of depth L (thread = node, its 256 children in order)
__global__ __launch_bounds__(256) void k_tr_assign(BwtArrays A, TrieArrays T, int L, int Dmax, int keys) {
  const int b = bw_row_block(A, blockIdx.x);
  const TrieView V = tr_view(T, b);
  int32_t* meta = V.meta;
  __shared__ u32 sNodes, sBuckets, sErr;
  __shared__ u32 scan[32];
  const int lo = (L == 1) ? 0 : meta[2 + L], hi = (L == 1) ? 256 : meta[10 + L];
  if (threadIdx.x == 0) { sNodes = (L == 1) ? 256u : (u32)meta[0]; sBuckets = (L == 1) ? 0u : (u32)meta[1]; sErr = 0; }
  __syncthreads();
  const u32 firstNew = sNodes;
  u32 *cnt = V.cnt, *info = V.info, *nodeStart = V.nodeStart, *bStart = V.bStart, *bCount = V.bCount, *bAux = V.bAux, *bG = V.bG;
  u32 *nodePfx = V.nodePfx, *nodeGS = V.nodeGS;
  const u32 skipTag = (u32)L << 16;                                      // packed next to a bucket's count (k_tr_sort reads it)
  for (int base = lo; base < hi; base += 256) {                          // uniform
    const int node = base + threadIdx.x;
    const bool valid = node < hi;
    u32 start = 0;
    if (L == 1) {                                                        // depth-1 nodes: their ranges from the byte totals
      u32 tot = 0;
      for (int c = 0; c < 256; c += 4) {
        const uint4 v = *(const uint4*)(cnt + (int64_t)node * 256 + c);
        tot += v.x + v.y + v.z + v.w;
      }
      u32 total;
      start = kz_wg_excl_sum(tot, scan, &total);
      nodeStart[node] = start;
      if (keys) nodePfx[node] = (u32)node;
    } else if (valid) start = nodeStart[node];
    if (!valid) continue;
    u32 run = start, curCnt = 0;
    int curB = -1;
    // key rounds (see k_trk_*): the first three key bytes are the old group g; a node of depth >= 3 knows g and where g's elements start
    const u32 pfxN = keys ? nodePfx[node] : 0u;
    const u32 gsN = (keys && L >= 3) ? nodeGS[node] : 0u;
    const u32 auxSmall = !keys ? 0u : (L >= 3 ? pfxN - gsN : pfxN);      // skip >= 3: slot = aux + position; skip < 3: the prefix bytes
    for (int c4 = 0; c4 < 256; c4 += 4) {
      const uint4 v4 = *(const uint4*)(cnt + (int64_t)node * 256 + c4);
      const u32 cc4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u32 cc = cc4[j];
        if (cc == 0) continue;
        const u32 s0 = run;
        run += cc;
        u32 e;
        const u32 cbyte = (u32)(c4 + j);
        if (cc > TR_CAP) {
          if (curB >= 0) { bCount[curB] = curCnt | skipTag; curB = -1; }
          if (L + 1 < Dmax) {
            const u32 M = atomicAdd(&sNodes, 1u);
            if (M < (u32)T.MN) {
              nodeStart[M] = s0; e = (TR_K_EXP << 30) | M;
              uint4* z = (uint4*)(cnt + (int64_t)M * 256);                // the new node's counters start at zero (no memset of the whole table)
              for (int q = 0; q < 64; q++) z[q] = make_uint4(0, 0, 0, 0);
              if (keys) { nodePfx[M] = (L < 3) ? ((pfxN << 8) | cbyte) : pfxN; nodeGS[M] = (L + 1 == 3) ? s0 : gsN; }
            } else { sErr = 1; e = (TR_K_TERM << 30) | s0; }
          } else if (keys) {                                              // all key bytes equal: one new group; its head slot = g + (s0 - group start)
            const u32 head = pfxN + (s0 - gsN);
            e = (TR_K_TERM << 30) | (s0 == gsN ? TR_UNCHANGED : 0u) | (head & 0xFFFFFFu);
          } else e = (TR_K_TERM << 30) | s0;
        } else if (cc > TR_MERGE) {
          if (curB >= 0) { bCount[curB] = curCnt | skipTag; curB = -1; }
          const u32 id = atomicAdd(&sBuckets, 1u);
          if (id < (u32)T.MB) { bStart[id] = s0; bCount[id] = cc | skipTag; bAux[id] = (keys && L >= 3) ? auxSmall + s0 : auxSmall; bG[id] = pfxN; } else sErr = 1;
          e = (TR_K_SMALL << 30) | ((u32)L << 16) | (id & 0xFFFFu);
        } else {
          if (curB >= 0 && curCnt + cc <= TR_CAP) curCnt += cc;
          else {
            if (curB >= 0) bCount[curB] = curCnt | skipTag;
            const u32 id = atomicAdd(&sBuckets, 1u);
            if (id < (u32)T.MB) { bStart[id] = s0; curB = (int)id; bAux[id] = (keys && L >= 3) ? auxSmall + s0 : auxSmall; bG[id] = pfxN; } else { sErr = 1; curB = -1; }
            curCnt = cc;
          }
          e = (TR_K_SMALL << 30) | ((u32)L << 16) | ((u32)curB & 0xFFFFu);
        }
        info[(int64_t)node * 256 + c4 + j] = e;
      }
    }
    if (curB >= 0) bCount[curB] = curCnt | skipTag;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    meta[0] = (int32_t)min(sNodes, (u32)T.MN); meta[1] = (int32_t)min(sBuckets, (u32)T.MB);
    meta[2 + L + 1] = (int32_t)firstNew; meta[10 + L + 1] = (int32_t)min(sNodes, (u32)T.MN);
    if (sErr) { meta[18] = 1; atomicOr(T.err, 1); }
  }
}

// level L >= 2: every suffix that is still inside an expanded node of depth L-1 looks its child up; children that were
// expanded (nodes of depth L) count the suffix's byte L in LDS.  state[i] = the suffix's leaf, or node | depth << 16.
#define TRC_U 4                  // quads of suffixes a thread keeps in flight
__global__ __launch_bounds__(1024) void k_tr_count(const u8* __restrict__ srcAll, int64_t stride, u32* __restrict__ stateAll, BwtArrays A, TrieArrays T, int L) {
  const int b = blockIdx.y;
  const TrieView V = tr_view(T, b);
  const int lo = V.meta[2 + L], hi = V.meta[10 + L];
  if (hi <= lo) return;                                                  // no node of this depth: the states stay as they are
  const int n = A.d_n[b];
  __shared__ u32 lds[TR_NODECHUNK * 256];
  const u8* s = srcAll + (int64_t)b * stride;
  u32* state = stateAll + (int64_t)b * A.NS;
  const u32* info = V.info;
  const int P = gridDim.x;
  const int per = (((n + P - 1) / P) + 1023) & ~1023;
  const int pbeg = blockIdx.x * per, pend = min(n, pbeg + per);
  for (int chunk = 0; lo + chunk * TR_NODECHUNK < hi; chunk++) {
    trc_zero_chunk(lds);
    const int nlo = lo + chunk * TR_NODECHUNK;
    // a thread takes four CONSECUTIVE suffixes: one 16-byte state access and one 8-byte text window serve all four, equal
    // targets in a row (runs) are added once; two such quads per thread are in flight (the chain state -> info -> counter is latency)
    for (int i0 = pbeg; i0 < pend; i0 += TRC_U * 4096) {
      uint4 st4[TRC_U]; u64 win[TRC_U]; bool any[TRC_U];
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        const int i = i0 + u * 4096 + threadIdx.x * 4;
        any[u] = i < pend;
        st4[u] = make_uint4(0xC0000000u, 0xC0000000u, 0xC0000000u, 0xC0000000u);
        win[u] = 0;
        if (any[u]) {
          if (!(L == 2 && chunk == 0)) st4[u] = *(const uint4*)(state + i);
          const int at = i + L - 2;                                        // bytes at .. at + 5: previous byte, child byte, counted byte of the four
          u64 k = __builtin_bswap64(*(const bw_u64_unaligned*)(s + at));
          const int rem = n - at;
          if (rem < 8) k = rem <= 0 ? 0ULL : (k & (~0ULL << (8 * (8 - rem))));
          win[u] = k;
        }
      }
      // the info lookups of ALL the quads are issued before any of them is used: one workgroup per CU (128 KiB of counters)
      // hides the chain state -> info -> counter only by what a thread keeps in flight
      u32 stqA[TRC_U][4]; u32 eA[TRC_U][4]; bool lookA[TRC_U][4];
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        const int i = i0 + u * 4096 + threadIdx.x * 4;
        stqA[u][0] = st4[u].x; stqA[u][1] = st4[u].y; stqA[u][2] = st4[u].z; stqA[u][3] = st4[u].w;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (L == 2 && chunk == 0) stqA[u][q] = (any[u] && i + q < pend) ? ((1u << 16) | (u32)((win[u] >> (56 - 8 * q)) & 0xFFu)) : 0xC0000000u;
          lookA[u][q] = any[u] && (i + q < pend) && (stqA[u][q] >> 30) == 0 && ((stqA[u][q] >> 16) & 7u) != (u32)L;
          eA[u][q] = 0;
          if (lookA[u][q]) eA[u][q] = info[(stqA[u][q] & 0xFFFFu) * 256 + (u32)((win[u] >> (48 - 8 * q)) & 0xFFu)];
        }
      }
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        if (!any[u]) continue;
        const int i = i0 + u * 4096 + threadIdx.x * 4;
        u32 (&stq)[4] = stqA[u];
        u32 cb[4];
#pragma unroll
        for (int q = 0; q < 4; q++) cb[q] = (u32)((win[u] >> (40 - 8 * q)) & 0xFFu);
        if (trc_resolve_quad(stq, eA[u], lookA[u], cb, pend - i, L, nlo, lds)) *(uint4*)(state + i) = make_uint4(stq[0], stq[1], stq[2], stq[3]);
      }
    }
    trc_flush_chunk(lds, V.cnt, nlo, hi);
  }
}

// move every suffix once (see above; tile and table sizes of the two forms: TRS_TILE / TRS_FASTB in kz_bwt_fwd.h)
template <int TILE_, int MAXB_, bool FAST>
__device__ __forceinline__ void tr_scatter_body(const u8* __restrict__ srcAll, int64_t stride, const u32* __restrict__ stateAll,
                                                u64* __restrict__ elemAll, const BwtArrays& A, const TrieArrays& T, int bitsG) {
  constexpr int ITEMS_ = TILE_ / 1024;
  if ((T.meta[(int64_t)blockIdx.y * TR_META + 1] <= TRS_FASTB) != FAST) return;
  const int b = blockIdx.y;
  const int n = A.d_n[b];
  const int tile = blockIdx.x;
  const int tbase = tile * TILE_;
  if (tbase >= n) return;
  __shared__ u32 tc2[MAXB_ / 2];                                       // two 16-bit counters per word
  __shared__ u32 gdelta[MAXB_];
  __shared__ u64 stage[TILE_];
  __shared__ uint16_t stageB[TILE_];
  __shared__ u32 scan[32];
  const TrieView V = tr_view(T, b);
  const int nB = V.meta[1];
  const bool hasState = V.meta[10 + 2] > V.meta[2 + 2];                  // a level-2 count pass wrote the states
  for (int i = threadIdx.x; i < (nB + 1) / 2; i += 1024) tc2[i] = 0;
  __syncthreads();
  const u8* s = srcAll + (int64_t)b * stride;
  const u32* state = stateAll + (int64_t)b * A.NS;
  const u32* info = V.info;
  u32* rank = A.rank + (int64_t)b * A.NS;
  const u64 lowMask = (1ULL << bitsG) - 1ULL;
  u64 el[ITEMS_]; u32 bp[ITEMS_];                                  // element, bucket | position in (tile, bucket) << 16
  // three rounds of loads for the tile's eight items per thread, each round issued for all items before its results are used
  // (state -> info -> text is a dependent chain; one item after the other was 24 memory round trips per thread, the kernel's time)
  u32 stv[ITEMS_];
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    stv[r] = 0xC0000000u;
    if (i < n) stv[r] = hasState ? state[i] : ((u32)s[i] | (1u << 16));
  }
  u32 cb[ITEMS_];
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    cb[r] = 0;
    if (i < n && (stv[r] >> 30) == 0) cb[r] = tr_byte(s, i + (int)((stv[r] >> 16) & 7u), n);
  }
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    if (i < n && (stv[r] >> 30) == 0) stv[r] = info[(stv[r] & 0xFFFFu) * 256 + cb[r]];
  }
  u64 kv[ITEMS_];
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    kv[r] = 0;
    if (i < n && (stv[r] >> 30) != TR_K_TERM) {
      const int at = i + (int)((stv[r] >> 16) & 7u);
      u64 k = __builtin_bswap64(*(const bw_u64_unaligned*)(s + at));
      const int rem = n - at;
      if (rem < 8) k = rem <= 0 ? 0ULL : (k & (~0ULL << (8 * (8 - rem))));
      kv[r] = k;
    }
  }
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    bp[r] = 0xFFFFFFFFu;
    el[r] = 0;
    if (i < n) {
      const u32 st = stv[r];
      if ((st >> 30) == TR_K_TERM) rank[i] = (st & 0xFFFFFFu) | BW_LIVE;
      else {
        const u32 bk = st & 0xFFFFu;
        el[r] = (kv[r] & ~lowMask) | (u64)(u32)i;
        bp[r] = tr_tile_place(tc2, bk);
      }
    }
  }
  tr_tile_flush<TILE_>(el, bp, nB, V, elemAll + (int64_t)b * A.NS, tc2, gdelta, stage, stageB, scan);
}

__global__ __launch_bounds__(1024) void k_tr_scatter(const u8* __restrict__ srcAll, int64_t stride, const u32* __restrict__ stateAll,
                                                      u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG) { tr_scatter_body<TRS_TILE, TR_MAXB, false>(srcAll, stride, stateAll, elemAll, A, T, bitsG); }
__global__ __launch_bounds__(1024) void k_tr_scatter_f(const u8* __restrict__ srcAll, int64_t stride, const u32* __restrict__ stateAll,
                                                        u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG) { tr_scatter_body<TRS_TILE / 2, TRS_FASTB, true>(srcAll, stride, stateAll, elemAll, A, T, bitsG); }

// round 0: a block whose trie has only the 256 depth-1 nodes (see the lazy ranks of k_tr_sort)
__device__ __forceinline__ bool tr_lazy_candidate(const int32_t* meta) { return meta[0] == 256 && meta[18] == 0; }
// one bucket at a time in LDS: sort by the key bits that differ, groups of equal keys, ranks and final suffixes
template <bool KEYS>
__device__ __forceinline__ void tr_sort_body(const u64* __restrict__ elemAll, const BwtArrays& A, const TrieArrays& T, int bitsG, int lazyMode) {
  const int b = bw_row_block(A, blockIdx.y);
  const int nB = T.meta[(int64_t)b * TR_META + 1];
  // LAZY RANKS (round 0 only).  A block without a single expanded node (no 2-byte prefix above TR_CAP suffixes: high-entropy data)
  // almost always leaves round 0 with every suffix final, and then nobody reads its ranks except k_bwt_emit (the 8 primary indexes):
  // the scattered 4-byte rank stores are a quarter of this kernel's time on such blocks.  Pass 1 (lazyMode 1) sorts such a block,
  // writes its final suffixes and the 8 ranks k_bwt_emit reads, and COUNTS the live suffixes in meta[20]; pass 2 (lazyMode 2) runs the
  // blocks whose count is not zero again, storing every rank (the elements are untouched by pass 1; the sa stores repeat).
  // k_live_emit skips the blocks pass 1 finished.
  const bool lazyCand = !KEYS && lazyMode != 0 && tr_lazy_candidate(T.meta + (int64_t)b * TR_META);
  if (!KEYS && lazyMode == 2 && !(lazyCand && T.meta[(int64_t)b * TR_META + 20] > 0)) return;
  const bool lazy = lazyCand && lazyMode == 1;
  u32 pstep = 0;
  if (lazy) { const int n = A.d_n[b]; const int st = n >> 3; pstep = (u32)((st * 8 != n) ? st + 1 : st); }   // k_bwt_emit: primary index k = rank[k * step]
  u32 liveMine = 0;
  __shared__ u64 buf[TR_CAP];
  __shared__ uint16_t cw[TRQ_WAVES][BK_DBINS];
  __shared__ u32 wsum[BK_DBINS / 64];
  __shared__ u32 wH[TRQ_WAVES], wS[TRQ_WAVES];
  __shared__ u64 redO[TRQ_WAVES], redA[TRQ_WAVES];
  __shared__ int skip[8];
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const int64_t off = (int64_t)b * A.NS;
  const u64* elem = elemAll + off;
  u32* rank = A.rank + off;
  u32* sa = A.sa + off;
  const uint64_t lt = kz_lanemask_lt();
  const uint64_t le = lt | (1ULL << lane);
  const u64 vmask = (1ULL << bitsG) - 1ULL;
  for (int d = blockIdx.x; d < nB; d += gridDim.x) {
    const u32 bcs = T.bCount[(int64_t)b * T.MB + d];
    const int cnt = (int)(bcs & 0xFFFFu);
    const int skipB = (int)(bcs >> 16);                                  // bytes of common prefix in front of the bucket's key fragment
    const u32 bo = T.bStart[(int64_t)b * T.MB + d];
    const u32 aux = KEYS ? T.bAux[(int64_t)b * T.MB + d] : 0u;
    const u32 gOne = KEYS ? T.bG[(int64_t)b * T.MB + d] : 0u;
    const int rows = (cnt + 63) >> 6;
    const int R = (rows + TRQ_WAVES - 1) / TRQ_WAVES;                    // rows per wave, 1..TRQ_ROWS (uniform)
    const int base = wave * R * 64;
    u64 k[TRQ_ROWS]; u32 dr[TRQ_ROWS];
    u64 vo = 0, va = ~0ULL;
#pragma unroll
    for (int r = 0; r < TRQ_ROWS; r++) {
      const int idx = base + r * 64 + lane;
      k[r] = ~0ULL;
      if (r < R && idx < cnt) { k[r] = elem[bo + idx]; vo |= k[r]; va &= k[r]; }
    }
    for (int dd = 32; dd > 0; dd >>= 1) { vo |= __shfl_xor(vo, dd, 64); va &= __shfl_xor(va, dd, 64); }
    if (threadIdx.x < 8) skip[threadIdx.x] = 0;
    if (lane == 0) { redO[wave] = vo; redA[wave] = va; }
    __syncthreads();
    vo = 0; va = ~0ULL;
#pragma unroll
    for (int w = 0; w < TRQ_WAVES; w++) { vo |= redO[w]; va &= redA[w]; }
    const u64 diff = (vo ^ va) >> bitsG;                                 // key bits that differ inside the bucket
    int passes = 0, lowBit = 0;
    if (diff) {
      lowBit = (int)__builtin_ctzll(diff);
      const int hiBit = 63 - (int)__builtin_clzll(diff);
      passes = (hiBit - lowBit + BK_DBITS) / BK_DBITS;
    }
    // (the LSD pass of bucket_body, kz_bwt_fwd.hip, as a second text: see the comment there.  This body also spells its table
    // pointers out instead of taking a tr_view: at the 64-VGPR cap any other text moves the spills)
    for (int p = 0; p < passes; p++) {
      const int shift = bitsG + lowBit + BK_DBITS * p;
      for (int i = threadIdx.x; i < TRQ_WAVES * BK_DBINS / 2; i += TRQ_WAVES * 64) ((u32*)&cw[0][0])[i] = 0;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < TRQ_ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          const bool valid = idx < cnt;
          const u32 dg = (u32)(k[r] >> shift) & (BK_DBINS - 1);
          const uint64_t vm = kz_ballot(valid);
          if (vm == 0) continue;
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
      static_assert(BK_DBINS <= TRQ_WAVES * 64, "one digit per thread");
      u32 mine = 0;                                                      // thread = digit (the threads behind carry zero)
      if (threadIdx.x < BK_DBINS) {
#pragma unroll
        for (int w = 0; w < TRQ_WAVES; w++) mine += cw[w][threadIdx.x];
        if (mine == (u32)cnt) skip[p] = 1;
      }
      const u32 inc = kz_wave_incl_sum(mine);
      if (lane == 63 && wave < BK_DBINS / 64) wsum[wave] = inc;
      __syncthreads();
      if (skip[p]) continue;                                             // uniform: one digit value for the whole bucket, nothing moves
      if (threadIdx.x < BK_DBINS) {
        u32 run = inc - mine;
        for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
        for (int w = 0; w < TRQ_WAVES; w++) { const u32 cv = cw[w][threadIdx.x]; cw[w][threadIdx.x] = (uint16_t)run; run += cv; }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < TRQ_ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          if (idx < cnt) buf[cw[wave][dr[r] & 0xFFFF] + (dr[r] >> 16)] = k[r];
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < TRQ_ROWS; r++) {
        if (r < R) {
          const int idx = base + r * 64 + lane;
          if (idx < cnt) k[r] = buf[idx];
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < TRQ_ROWS; r++) {
      if (r < R) {
        const int idx = base + r * 64 + lane;
        if (idx < cnt) buf[idx] = k[r];
      }
    }
    __syncthreads();
    // groups of equal keys; key rounds with skip < 3 also need the OLD groups (the first 3 - skip key bytes): an element's slot
    // is g + its index inside its old group, a new group's rank g + the index of its first element inside the old group
    // (NOT shared with bucket_body's group heads, on purpose: that one keeps the rows' ballots in registers between its two loops,
    // this one computes them twice -- k_tr_sort / k_trk_sort sit at the 64-VGPR cap of two workgroups per CU and spill as it is)
    const bool segs = KEYS && skipB < 3;
    const int gsh = 64 - 8 * (3 - skipB);                                 // element >> gsh = the bytes of g the fragment holds
    u32 mh = 0, ms = 0;
#pragma unroll
    for (int r = 0; r < TRQ_ROWS; r++) {
      if (r < R) {
        const int idx = base + r * 64 + lane;
        const bool valid = idx < cnt;
        const u64 prev = (valid && idx > 0) ? buf[idx - 1] : 0;
        const bool head = valid && (idx == 0 || (k[r] >> bitsG) != (prev >> bitsG));
        const uint64_t hbr = kz_ballot(head);
        if (hbr) mh = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(hbr)) + 1;
        if (segs) {
          const uint64_t sbr = kz_ballot(head && (idx == 0 || (k[r] >> gsh) != (prev >> gsh)));
          if (sbr) ms = (u32)(base + r * 64 + 63 - (int)__builtin_clzll(sbr)) + 1;
        }
      }
    }
    if (lane == 0) { wH[wave] = mh; wS[wave] = ms; }
    __syncthreads();
    u32 carH = 0, carS = 0;
    for (int w = 0; w < wave; w++) { carH = max(carH, wH[w]); carS = max(carS, wS[w]); }
#pragma unroll
    for (int r = 0; r < TRQ_ROWS; r++) {
      if (r < R) {
        const int rowBase = base + r * 64;
        const int idx = rowBase + lane;
        const bool valid = idx < cnt;
        const u64 prev = (valid && idx > 0) ? buf[idx - 1] : 0;
        const bool head = valid && (idx == 0 || (k[r] >> bitsG) != (prev >> bitsG));
        const uint64_t hbr = kz_ballot(head);
        const uint64_t hbl = hbr & le;
        const u32 hh = hbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(hbl)) : carH - 1;
        uint64_t sbr = 0;
        u32 ss = 0;
        if (segs) {
          sbr = kz_ballot(head && (idx == 0 || (k[r] >> gsh) != (prev >> gsh)));
          const uint64_t sbl = sbr & le;
          ss = sbl ? (u32)(rowBase + 63 - (int)__builtin_clzll(sbl)) : carS - 1;
        }
        if (valid) {
          const u64 nextk = (idx + 1 < cnt) ? buf[idx + 1] : 0;
          const bool headN = (idx + 1 >= cnt) || ((nextk >> bitsG) != (k[r] >> bitsG));
          const bool live = !(hh == (u32)idx && headN);
          const u32 sv = (u32)(k[r] & vmask);
          if (!KEYS) {
            if (!lazy) rank[sv] = (bo + hh) | (live ? BW_LIVE : 0u);
            else {
              const u32 q = sv / pstep;
              if (q * pstep == sv && q < 8u) rank[sv] = (bo + hh) | (live ? BW_LIVE : 0u);
              liveMine += live ? 1u : 0u;
            }
            if (!live) sa[bo + (u32)idx] = sv;
          } else {
            u32 g, headSlot, slot;
            if (segs) {
              g = (aux << (8 * (3 - skipB))) | (u32)(k[r] >> gsh);
              headSlot = g + (hh - ss); slot = g + ((u32)idx - ss);
            } else { g = gOne; headSlot = aux + hh; slot = aux + (u32)idx; }
            // the first new group of an old group keeps the old head slot: while it stays LIVE its members' ranks do not change
            if (!(live && headSlot == g)) rank[sv] = headSlot | (live ? BW_LIVE : 0u);
            if (!live) sa[slot] = sv;
          }
        }
        if (hbr) carH = (u32)(rowBase + 63 - (int)__builtin_clzll(hbr)) + 1;
        if (sbr) carS = (u32)(rowBase + 63 - (int)__builtin_clzll(sbr)) + 1;
      }
    }
    __syncthreads();
  }
  if (!KEYS && lazy) {
    if (kz_ballot(liveMine != 0) != 0) {
      for (int dd = 32; dd > 0; dd >>= 1) liveMine += __shfl_xor(liveMine, dd, 64);
      if (lane == 0) atomicAdd(&T.meta[(int64_t)b * TR_META + 20], (int32_t)liveMine);
    }
  }
}
// (two workgroups per CU at 64 VGPRs with 16 registers spilled beat one workgroup without spills: 45 vs 50 ms per 357 uniform blocks)
__global__ __launch_bounds__(1024, 8) void k_tr_sort(const u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG, int lazyMode) { tr_sort_body<false>(elemAll, A, T, bitsG, lazyMode); }
__global__ __launch_bounds__(1024, 8) void k_trk_sort(const u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG) { tr_sort_body<true>(elemAll, A, T, bitsG, 0); }

// ---------------------------------------------------------------------------------------------
// KEY rounds: the same trie round over the WINDOW of a doubling round -- the compact pairs (old group g << bitsR | secondary key r2,
// suffix) of the buckets too large for the LDS kernels (groups of many thousand suffixes: six full LSD passes over HBM and the
// k_seg_* kernels until round 3).  The digits are the six bytes of K48 = g : 24 | r2 : 24; the first three bytes are the old
// group, so a child of depth 3 IS an old group and its start in the sorted window is where the group's elements begin: an
// element at sorted position pos of group g takes slot g + (pos - group start).  A child that is still large after all six
// bytes holds equal keys only: one new group, no sorting (terminal).  Buckets of merged small siblings above depth 3 hold whole
// old groups (k_trk_sort finds their boundaries in the sorted fragment), buckets below depth 3 lie inside one group.
struct KeySrc { const u64* key; const u32* val; int bitsR; };
__device__ __forceinline__ u64 trk_k48(u64 key, int bitsR) { return ((key >> bitsR) << 24) | (key & ((1ULL << bitsR) - 1ULL)); }

__global__ __launch_bounds__(1024) void k_trk_hist16(KeySrc X, BwtArrays A, TrieArrays T) {
  const int b = bw_row_block(A, blockIdx.y);
  const int w0 = A.d_w[b];
  const int W = max(0, A.d_m[b] - w0);                                  // an empty window still writes its (zero) counts: k_tr_assign reads them
  const u32 half = blockIdx.x;
  __shared__ u32 hist[32768];
  trc_zero_chunk(hist);
  const u64* key = X.key + (int64_t)b * A.NS + w0;
  const int lane = kz_lane();
  for (int j0 = 0; j0 < W; j0 += 1024) {
    const int j = j0 + threadIdx.x;
    u32 tgt = 0xFFFFFFFFu;
    if (j < W) {
      const u32 pair = (u32)(trk_k48(key[j], X.bitsR) >> 32);
      if ((pair >> 15) == half) tgt = pair & 32767u;
    }
    const uint64_t am = kz_ballot(tgt != 0xFFFFFFFFu);                   // the window is grouped by bucket: most rows hit one counter
    if (am) {
      const int l0 = (int)__builtin_ctzll(am);
      const u32 t0 = (u32)__shfl((int)tgt, l0, 64);
      const uint64_t same = kz_ballot(tgt == t0);
      if (lane == l0) atomicAdd(&hist[t0], (u32)__popcll(same));
      else if (tgt != 0xFFFFFFFFu && tgt != t0) atomicAdd(&hist[tgt], 1u);
    }
  }
  tr_hist16_flush(hist, tr_view(T, b).cnt + half * 32768);
}

__global__ __launch_bounds__(1024) void k_trk_count(KeySrc X, u32* __restrict__ stateAll, BwtArrays A, TrieArrays T, int L) {
  const int b = bw_row_block(A, blockIdx.y);
  const TrieView V = tr_view(T, b);
  const int lo = V.meta[2 + L], hi = V.meta[10 + L];
  if (hi <= lo) return;
  const int w0 = A.d_w[b];
  const int W = A.d_m[b] - w0;
  __shared__ u32 lds[TR_NODECHUNK * 256];
  const u64* key = X.key + (int64_t)b * A.NS + w0;
  u32* state = stateAll + (int64_t)b * A.NS;
  const u32* info = V.info;
  const int P = gridDim.x;
  const int per = (((W + P - 1) / P) + 1023) & ~1023;
  const int pbeg = blockIdx.x * per, pend = min(W, pbeg + per);
  for (int chunk = 0; lo + chunk * TR_NODECHUNK < hi; chunk++) {
    trc_zero_chunk(lds);
    const int nlo = lo + chunk * TR_NODECHUNK;
    // a thread takes four CONSECUTIVE items (two 16-byte key loads, one 16-byte state access); equal targets in a row are added once;
    // TRC_U such quads are in flight per thread: all their loads, then all their info lookups, then the counters
    for (int i0 = pbeg; i0 < pend; i0 += TRC_U * 4096) {
      u64 kq[TRC_U][4]; u32 stq[TRC_U][4]; bool act[TRC_U];
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        const int i = i0 + u * 4096 + (int)threadIdx.x * 4;
        act[u] = i < pend;
#pragma unroll
        for (int q = 0; q < 4; q++) { stq[u][q] = 0xC0000000u; kq[u][q] = 0; }
        if (!act[u]) continue;
        if (!(L == 2 && chunk == 0)) {                                     // settled items (most of a late level's window) cost one state read
          const uint4 sv = *(const uint4*)(state + i);
          stq[u][0] = sv.x; stq[u][1] = sv.y; stq[u][2] = sv.z; stq[u][3] = sv.w;
          if ((stq[u][0] >> 30) && (stq[u][1] >> 30) && (stq[u][2] >> 30) && (stq[u][3] >> 30)) { act[u] = false; continue; }
        }
        if (i + 4 <= pend && ((((uintptr_t)(key + i)) & 15) == 0)) {
          const uint4 a = *(const uint4*)(key + i), c = *(const uint4*)(key + i + 2);
          kq[u][0] = ((u64)a.y << 32) | a.x; kq[u][1] = ((u64)a.w << 32) | a.z; kq[u][2] = ((u64)c.y << 32) | c.x; kq[u][3] = ((u64)c.w << 32) | c.z;
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++) kq[u][q] = (i + q < pend) ? key[i + q] : 0ULL;
        }
      }
      u32 e[TRC_U][4]; bool look[TRC_U][4]; u64 k48[TRC_U][4];
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        const int i = i0 + u * 4096 + (int)threadIdx.x * 4;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          k48[u][q] = trk_k48(kq[u][q], X.bitsR);
          if (L == 2 && chunk == 0) stq[u][q] = (act[u] && i + q < pend) ? ((1u << 16) | (u32)(k48[u][q] >> 40)) : 0xC0000000u;
          look[u][q] = act[u] && (i + q < pend) && (stq[u][q] >> 30) == 0 && ((stq[u][q] >> 16) & 7u) != (u32)L;
          e[u][q] = 0;
          if (look[u][q]) e[u][q] = info[(stq[u][q] & 0xFFFFu) * 256 + (u32)((k48[u][q] >> (40 - 8 * (L - 1))) & 0xFFu)];
        }
      }
#pragma unroll
      for (int u = 0; u < TRC_U; u++) {
        if (!act[u]) continue;
        const int i = i0 + u * 4096 + (int)threadIdx.x * 4;
        u32 cb[4];
#pragma unroll
        for (int q = 0; q < 4; q++) cb[q] = (u32)((k48[u][q] >> (40 - 8 * L)) & 0xFFu);
        if (trc_resolve_quad(stq[u], e[u], look[u], cb, pend - i, L, nlo, lds)) *(uint4*)(state + i) = make_uint4(stq[u][0], stq[u][1], stq[u][2], stq[u][3]);
      }
    }
    trc_flush_chunk(lds, V.cnt, nlo, hi);
  }
}

template <int TILE_, int MAXB_, bool FAST>
__device__ __forceinline__ void trk_scatter_body(const KeySrc& X, const u32* __restrict__ stateAll, u64* __restrict__ elemAll, const BwtArrays& A, const TrieArrays& T, int bitsG) {
  constexpr int ITEMS_ = TILE_ / 1024;
  const int b = bw_row_block(A, blockIdx.y);
  if ((T.meta[(int64_t)b * TR_META + 1] <= TRS_FASTB) != FAST) return;
  const int w0 = A.d_w[b];
  const int W = A.d_m[b] - w0;
  const int tbase = blockIdx.x * TILE_;
  if (tbase >= W) return;
  __shared__ u32 tc2[MAXB_ / 2];
  __shared__ u32 gdelta[MAXB_];
  __shared__ u64 stage[TILE_];
  __shared__ uint16_t stageB[TILE_];
  __shared__ u32 scan[32];
  const TrieView V = tr_view(T, b);
  const int nB = V.meta[1];
  const bool hasState = V.meta[10 + 2] > V.meta[2 + 2];
  for (int i = threadIdx.x; i < (nB + 1) / 2; i += 1024) tc2[i] = 0;
  __syncthreads();
  const u64* key = X.key + (int64_t)b * A.NS + w0;
  const u32* val = X.val + (int64_t)b * A.NS + w0;
  const u32* state = stateAll + (int64_t)b * A.NS;
  const u32* info = V.info;
  u32* rank = A.rank + (int64_t)b * A.NS;
  const u64 lowMask = (1ULL << bitsG) - 1ULL;
  u64 el[ITEMS_]; u32 bp[ITEMS_];
  // loads in rounds, as in k_tr_scatter: keys / suffixes / states of all items, then all info lookups
  u64 k48v[ITEMS_]; u32 svv[ITEMS_], stv[ITEMS_];
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    k48v[r] = 0; svv[r] = 0; stv[r] = 0xC0000000u;
    if (i < W) {
      k48v[r] = trk_k48(key[i], X.bitsR);
      svv[r] = val[i];
      stv[r] = hasState ? state[i] : ((1u << 16) | (u32)(k48v[r] >> 40));
    }
  }
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    if (i < W && (stv[r] >> 30) == 0) stv[r] = info[(stv[r] & 0xFFFFu) * 256 + (u32)((k48v[r] >> (40 - 8 * (int)((stv[r] >> 16) & 7u))) & 0xFFu)];
  }
#pragma unroll
  for (int r = 0; r < ITEMS_; r++) {
    const int i = tbase + r * 1024 + threadIdx.x;
    bp[r] = 0xFFFFFFFFu;
    el[r] = 0;
    if (i < W) {
      const u64 k48 = k48v[r];
      const u32 sv = svv[r];
      const u32 st = stv[r];
      if ((st >> 30) == TR_K_TERM) {                                       // a new group of equal keys: its members' ranks, nothing to sort
        if (!(st & TR_UNCHANGED)) rank[sv] = (st & 0xFFFFFFu) | BW_LIVE;
      } else {
        const u32 bk = st & 0xFFFFu;
        const int skip = (int)((st >> 16) & 7u);
        el[r] = (((k48 << 16) << (8 * skip)) & ~lowMask) | (u64)sv;
        bp[r] = tr_tile_place(tc2, bk);
      }
    }
  }
  tr_tile_flush<TILE_>(el, bp, nB, V, elemAll + (int64_t)b * A.NS, tc2, gdelta, stage, stageB, scan);
}

__global__ __launch_bounds__(1024) void k_trk_scatter(KeySrc X, const u32* __restrict__ stateAll, u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG) { trk_scatter_body<TRS_TILE, TR_MAXB, false>(X, stateAll, elemAll, A, T, bitsG); }
__global__ __launch_bounds__(1024) void k_trk_scatter_f(KeySrc X, const u32* __restrict__ stateAll, u64* __restrict__ elemAll, BwtArrays A, TrieArrays T, int bitsG) { trk_scatter_body<TRS_TILE / 2, TRS_FASTB, true>(X, stateAll, elemAll, A, T, bitsG); }

// ---------------------------------------------------------------------------------------------
// The trie round is used for blocks of 64 KiB .. 4 MiB (+ slack).  Table bounds (n = block length, C = TR_CAP):
//   nodes: 256 of depth 1 + at most n / (C + 1) expanded children per level, levels 2 .. TR_DMAX_LIMIT - 1;
//   buckets: children above TR_MERGE (<= n / (TR_MERGE + 1)) + merged ones: two neighbours of a run hold more than C suffixes
//   together (<= 2n / C + 1 per run) and a run starts at a node or behind a breaker (nodes + children above TR_MERGE + terminals).
static inline int tr_max_nodes(int maxN) { return 257 + (TR_DMAX_LIMIT - 2) * (maxN / (int)(TR_CAP + 1) + 1); }
static inline int tr_max_buckets(int maxN) {
  const int med = maxN / (int)(TR_MERGE + 1) + 1, big = maxN / (int)(TR_CAP + 1) + 1;
  return med + 2 * (maxN / (int)TR_CAP) + 2 + tr_max_nodes(maxN) + med + (TR_DMAX_LIMIT - 2) * big + big;
}
bool tr_applies(int maxN) {                          // (KZ_BWT_TRIE=0 switches the trie rounds off at the call: ctx->sw.bwtTrie)
  return maxN >= TR_MIN_N && maxN <= TR_MAX_N && tr_max_buckets(maxN) <= TR_MAXB && tr_max_nodes(maxN) <= 65535;
}

// the tables of one block, in bytes (bwt_trie_alloc below takes exactly these, B times)
size_t bwt_trie_scratch(int maxN) {
  const size_t MN = (size_t)tr_max_nodes(maxN), MB = TR_MAXB;
  return MN * 256 * 4 * 2        // cnt, info
       + MN * 4 * 3              // nodeStart, nodePfx, nodeGS
       + MB * 4 * 5              // bStart, bCount, bFill, bAux, bG
       + TR_META * 4             // meta
       + 9 * 256;                // err, and the allocations' alignment
}
bool bwt_trie_alloc(kz_ctx* ctx, int B, int maxN, TrieArrays& TR) {
  const size_t mark = ctx->arenaTop;
  TR.MN = tr_max_nodes(maxN); TR.MB = TR_MAXB;
  const size_t MN = (size_t)B * TR.MN, MB = (size_t)B * TR.MB;
  auto words = [&](size_t n) { return (u32*)kz_arena_alloc(ctx, n * 4); };
  TR.cnt = words(MN * 256); TR.info = words(MN * 256); TR.nodeStart = words(MN);
  TR.bStart = words(MB); TR.bCount = words(MB); TR.bFill = words(MB); TR.bAux = words(MB); TR.bG = words(MB);
  TR.nodePfx = words(MN); TR.nodeGS = words(MN);
  TR.meta = (int32_t*)words((size_t)B * TR_META);
  TR.err = (int32_t*)kz_arena_alloc(ctx, 256);
  if (TR.cnt && TR.info && TR.nodeStart && TR.bStart && TR.bCount && TR.bFill && TR.bAux && TR.bG && TR.nodePfx && TR.nodeGS && TR.meta && TR.err) return true;
  ctx->arenaTop = mark;
  return false;
}

// ---- the trie round over the text: count level by level, move once, finish the buckets in LDS (elements in key[0], states in val[0]) ----
int bwt_trie_text_round(BwtRun& R) {
  kz_ctx* ctx = R.ctx;
  const BwtArrays& A = R.A; const TrieArrays& TR = R.TR;
  const int B = R.B;
  const u8* src = R.bt->buf[R.bt->cur];
  const int64_t stride = R.bt->stride;
  KZ_HIP(hipMemsetAsync(TR.bFill, 0, (size_t)B * TR.MB * 4, ctx->stream));
  KZ_HIP(hipMemsetAsync(TR.meta, 0, (size_t)B * TR_META * 4, ctx->stream));
  KZ_LAUNCH(ctx, KID_TR_HIST16, k_tr_hist16, dim3(2, B), dim3(1024), src, stride, A, TR);
  KZ_LAUNCH(ctx, KID_TR_ASSIGN, k_tr_assign, dim3(B), dim3(256), A, TR, 1, R.Dmax, 0);
  const int P = B >= 2048 ? 1 : (B >= 1024 ? 2 : 8);
  for (int L = 2; L < R.Dmax; L++) {
    KZ_LAUNCH(ctx, KID_TR_COUNT, k_tr_count, dim3(P, B), dim3(1024), src, stride, A.val[0], A, TR, L);
    KZ_LAUNCH(ctx, KID_TR_ASSIGN, k_tr_assign, dim3(B), dim3(256), A, TR, L, R.Dmax, 0);
  }
  KZ_LAUNCH(ctx, KID_TR_SCATTER, k_tr_scatter_f, dim3(gridFor(R.maxN, TRS_TILE / 2), B), dim3(1024), src, stride, A.val[0], A.key[0], A, TR, R.bitsG);
  KZ_LAUNCH(ctx, KID_TR_SCATTER, k_tr_scatter, dim3(gridFor(R.maxN, TRS_TILE), B), dim3(1024), src, stride, A.val[0], A.key[0], A, TR, R.bitsG);
  const int G = std::max(16, std::min(1024, 8192 / B));
  KZ_LAUNCH(ctx, KID_TR_SORT, k_tr_sort, dim3(G, B), dim3(1024), A.key[0], A, TR, R.bitsG, R.lazyRank ? 1 : 0);
  if (R.lazyRank) KZ_LAUNCH(ctx, KID_TR_SORT, k_tr_sort, dim3(G, B), dim3(1024), A.key[0], A, TR, R.bitsG, 2);   // the blocks pass 1 guessed wrong (workgroups of the others leave at once)
  return 0;
}

// ---- the window of oversized buckets through a KEY trie round (k_trk_*): count by key byte, move once, finish in LDS ----
int bwt_trie_key_round(BwtRun& R) {
  kz_ctx* ctx = R.ctx;
  const BwtArrays& A = R.A; const TrieArrays& TR = R.TR;
  const int nAct = R.nAct;
  const KeySrc XK = {R.kC, R.vC, R.bitsR};
  KZ_HIP(hipMemsetAsync(TR.bFill, 0, (size_t)R.B * TR.MB * 4, ctx->stream));
  KZ_HIP(hipMemsetAsync(TR.meta, 0, (size_t)R.B * TR_META * 4, ctx->stream));
  KZ_LAUNCH(ctx, KID_TR_HIST16, k_trk_hist16, dim3(2, nAct), dim3(1024), XK, A, TR);
  KZ_LAUNCH(ctx, KID_TR_ASSIGN, k_tr_assign, dim3(nAct), dim3(256), A, TR, 1, 6, 1);
  const int PW = nAct >= 1024 ? 1 : (nAct >= 256 ? 2 : 4);
  for (int L = 2; L < 6; L++) {
    KZ_LAUNCH(ctx, KID_TR_COUNT, k_trk_count, dim3(PW, nAct), dim3(1024), XK, R.vF, A, TR, L);
    KZ_LAUNCH(ctx, KID_TR_ASSIGN, k_tr_assign, dim3(nAct), dim3(256), A, TR, L, 6, 1);
  }
  KZ_LAUNCH(ctx, KID_TR_SCATTER, k_trk_scatter_f, dim3(gridFor(R.wMax, TRS_TILE / 2), nAct), dim3(1024), XK, R.vF, R.kF, A, TR, R.bitsG);
  KZ_LAUNCH(ctx, KID_TR_SCATTER, k_trk_scatter, dim3(gridFor(R.wMax, TRS_TILE), nAct), dim3(1024), XK, R.vF, R.kF, A, TR, R.bitsG);
  const int G = std::max(16, std::min(1024, 8192 / nAct));
  KZ_LAUNCH(ctx, KID_TR_SORT, k_trk_sort, dim3(G, nAct), dim3(1024), R.kF, A, TR, R.bitsG);
  return 0;
}
