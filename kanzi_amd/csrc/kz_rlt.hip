// kz_rlt.hip -- RLT, the escaped run-length transform, on gfx950 (scan-based, tile-parallel, many blocks per launch).
//
// Replaces K/transform/RLT.java:69-266 (forward) and :302-410 (inverse), bit for bit, the verdict included.
//
// FORWARD.  The reference walks the block: byte 0 goes out in the header (escape, byte 0, and a 0 when byte 0 is the escape,
// :152-158); then it counts the bytes equal to `prev` four at a time and closes a SEGMENT when fewer than four match, when the count
// reaches MAX_RUN4 = 73 469 or when srcIdx reaches srcEnd4 = n - 4 (:161-183).  A segment of more than three counted bytes is coded
// `prev, [0 if prev is the escape], escape, length` (:185-197, length in 1-3 bytes, :276-292), a shorter one is copied with escapes
// doubled (:198-216).  So a maximal run of equal bytes that starts at s is cut into pieces at s + 73 469 j (s = 0: the first piece has
// 73 473 bytes, byte 0 not being counted), and every piece boundary is a function of the run's start alone.  The loop ends at the
// first piece head q >= n - 5 (:222); from there on everything is copied, escapes doubled (:226-260).
//
// Parallel form, one lane per byte, rows of 64 as in kz_zrlt.hip.  A lane knows the start of the run it is in (a max-scan of
// "last position whose byte differs from the one before": ballot inside a row, LDS between the waves of a tile, k_rlt_fscan over
// the tiles), hence its piece and its place in it, and sees the next bytes through the row's ballot mask.  A coded piece is emitted by
// the lane of its LAST byte, a copied byte by its own lane; offsets are an exclusive sum-scan of the sizes.  The piece that holds
// byte n - 5 is the only one the end of the block can cut (every earlier one ends at or before n - 5): its bytes and everything
// behind them belong to one lane per block in k_rlt_ftail, which sizes the piece in closed form (its head from the run's start, its
// end from at most four bytes ahead) and then runs the reference's tail as written -- at most 5 source bytes by a serial walk.
// The reference's bound checks (:186, :199, :207) compare dstIdx with dstEnd = dst.length: with the exclusive scan they are per-lane
// comparisons and the verdict is their OR (after the first failure the result is "false" whatever follows).
//
// kernels: k_rlt_f0 (last boundary per tile; the order-0 histogram when the escape is searched) -> k_rlt_fscan (per block: type rules,
// escape, run start per tile) -> k_rlt_f1 (sizes per tile) -> k_rlt_fsum (offsets per tile) -> k_rlt_f3 (emit) -> k_rlt_ftail.
// Three passes over the input.
//
// INVERSE.  What a byte means (literal / escape mark / first, second, third length byte) is the state of a five-state machine driven by
// the bytes before it.  A thread takes 16 consecutive bytes and composes their transition maps (5 x 3 bits), a wave scan and LDS give
// the map of a tile (k_rlt_i1), k_rlt_iscan the state at every tile's start.  With the states known a thread walks its 16 bytes as the
// reference does: token sizes (k_rlt_i2), offsets by sum-scan (k_rlt_isum), then the bytes (k_rlt_i3).  A run repeats dst[dstIdx - 1],
// the last byte PRODUCED (:353): the value of the last literal / escape literal token, carried by a max-scan of (position, value);
// runs of 32 bytes and more are written by all lanes of the wave with 16-byte stores.
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_datatype.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

#define RL_TILE (KZ_WG * 16)             // bytes per workgroup
#define RL_WROWS 16                      // rows of 64 bytes per wave
#define RL_PIECE 73469u                  // MAX_RUN4 (:37): a piece of a run that does not start the block
#define RL_PIECE0 73473u                 // the first piece of a run that starts the block (byte 0 is not counted, :152-153)
#define RL_ENC1 224u                     // RUN_LEN_ENCODE1 (:32)
#define RL_ENC2 7936u                    // RUN_LEN_ENCODE2 (:33)
static_assert(RL_TILE == (KZ_WG / 64) * RL_WROWS * 64, "RLT tile geometry");

struct RlScratch {
  u32* tLastB;     // [B][T] position + 1 of the tile's last boundary (a byte that differs from the one before; byte 0 is one), 0: none
  u32* tS;         // [B][T] position + 1 of the last boundary before the tile
  u32* tSum;       // [B][T] output bytes of the tile's lanes
  u32* tOff;       // [B][T] exclusive sum of tSum
  u32* hist;       // [B][256] order-0 histogram (escape search only)
  u32* s5;         // [B] start of the run that holds byte n - 5
  int32_t* esc;    // [B]
  int32_t* decl;   // [B] 1: declined before any byte was looked at (length, data type)
  int32_t* fail;   // [B]
  int32_t* total;  // [B] output bytes in front of the tail lane's
  const int32_t* dstEnd;   // [B] or null
  int dstEndAll;
  int T;
};

// head of the piece that holds byte i of the run that starts at s
__device__ __forceinline__ u32 rl_head(u32 s, u32 i) {
  const u32 d = i - s;
  const u32 first = (s == 0u) ? RL_PIECE0 : RL_PIECE;
  if (d < first) return s;
  return s + first + ((d - first) / RL_PIECE) * RL_PIECE;
}
__device__ __forceinline__ u32 rl_len_bytes(u32 run) {                  // emitRunLength :276-292
  const u32 r = run - 3u;
  return (r < RL_ENC1) ? 1u : ((r < RL_ENC2) ? 2u : 3u);
}
__device__ __forceinline__ u32 rl_emit_len(u8* o, u32 idx, u32 run) {
  u32 r = run - 3u;
  if (r >= RL_ENC1) {
    if (r < RL_ENC2) { r -= RL_ENC1; o[idx++] = (u8)(RL_ENC1 + (r >> 8)); }
    else { r -= RL_ENC2; o[idx++] = 0xFF; o[idx++] = (u8)(r >> 8); }
  }
  o[idx] = (u8)r;
  return idx + 1u;
}

// What lane i (0 <= i <= n - 6) puts out: its size, and *run > 0 when it is the coded piece that ends at i.
//   s: start of the run i is in; v: its byte; z: how many of the bytes behind i equal it (exact up to 4).
__device__ __forceinline__ u32 rl_item(u32 i, u32 n, u32 s, u32 v, u32 z, u32 esc, u32* run) {
  *run = 0u;
  const u32 w = (v == esc) ? 2u : 1u;
  if (i == 0u) return 1u + w;                                            // the header :154-158
  const u32 d = i - s;
  const u32 first = (s == 0u) ? RL_PIECE0 : RL_PIECE;
  u32 p = s;
  bool cutNext = false;                                                  // byte i + 1 heads the next piece of the same run
  if (d + 1u == first) cutNext = true;
  else if (d + 1u > first) { const u32 dd = d - first; p = s + first + (dd / RL_PIECE) * RL_PIECE; cutNext = ((dd + 1u) % RL_PIECE) == 0u; }
  const u32 e = i - p;
  const u32 thr = (p == 0u) ? 4u : 3u;                                   // the piece is coded when it reaches this offset (run > 3, :185)
  // the piece that holds byte n - 5 is the tail lane's; a lane further from the end than this is in the coded part of such a piece
  if (i + 9u >= n) { const u32 k = n - 5u - i; if (z >= k && rl_head(s, n - 5u) == p) return 0u; }
  if (e >= thr) {
    if (z != 0u && !cutNext) return 0u;
    *run = (p == 0u) ? e : e + 1u;
    return w + 1u + rl_len_bytes(*run);
  }
  return (z >= thr - e) ? 0u : w;                                        // (no cut this close to the piece's head)
}

// the tile, one byte before it and 16 behind it -> LDS (zeros behind the block's end); then per wave the boundary masks of its 16 rows
// and of the 8 bytes behind them
#define RL_LOAD_ROWS(INB)                                                                                 \
  {                                                                                                       \
    const int p16 = tstart + 16 * (int)threadIdx.x;                                                       \
    uint4 q = make_uint4(0u, 0u, 0u, 0u);                                                                 \
    if (p16 + 16 <= n) q = *(const uint4*)(s + p16);                                                      \
    else if (p16 < n) { u8 tb[16]; for (int k = 0; k < 16; k++) tb[k] = (p16 + k < n) ? s[p16 + k] : (u8)0; memcpy(&q, tb, 16); } \
    ((uint4*)(INB))[1 + threadIdx.x] = q;                                                                 \
    if (threadIdx.x < 16) { const int g = tstart + RL_TILE + (int)threadIdx.x; (INB)[16 + RL_TILE + threadIdx.x] = (g < n) ? s[g] : (u8)0; } \
    if (threadIdx.x == 16) (INB)[15] = (tstart > 0) ? s[tstart - 1] : (u8)0;                              \
  }                                                                                                       \
  __syncthreads();                                                                                        \
  u32 v[RL_WROWS]; u64 bnd[RL_WROWS + 1];                                                                 \
  u32 myLast = 0;                                             /* position + 1 of the wave's last boundary */ \
  _Pragma("unroll") for (int r = 0; r <= RL_WROWS; r++) {                                                 \
    const int pos = wbase + 64 * r + lane;                                                                \
    bool bd = true;                                                                                       \
    if (r < RL_WROWS || lane < 8) {                                                                       \
      const u32 cur = (u32)(INB)[16 + pos - tstart], prv = (u32)(INB)[15 + pos - tstart];                 \
      if (r < RL_WROWS) v[r] = cur;                                                                       \
      bd = (pos == 0) || (pos >= n) || (cur != prv);                                                      \
    }                                                                                                     \
    bnd[r] = kz_ballot(bd);                                                                               \
    if (r < RL_WROWS) { const u64 in = bnd[r] & rowValid(wbase + 64 * r, n); if (in) myLast = (u32)(wbase + 64 * r + 64 - (int)__builtin_clzll(in)); } \
  }

__device__ __forceinline__ u64 rowValid(int rowBase, int n) {            // lanes of the row that are inside the block
  const int k = n - rowBase;
  return (k >= 64) ? ~0ULL : ((k <= 0) ? 0ULL : ((1ULL << k) - 1ULL));
}

// ---- forward 0: last boundary per tile, histogram ----------------------------------------------------------------------------
__global__ __launch_bounds__(KZ_WG) void k_rlt_f0(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, RlScratch S, int doHist) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RL_TILE;
  if (tstart >= n) return;
  const u8* s = src + (int64_t)b * stride;
  const int pos = tstart + 16 * (int)threadIdx.x;
  __shared__ u32 h[256];
  __shared__ u32 wl[KZ_WG / 64];
  if (doHist) h[threadIdx.x] = 0;
  u8 tb[16];
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (pos + 16 <= n) q = *(const uint4*)(s + pos);
  else if (pos < n) { for (int k = 0; k < 16; k++) tb[k] = (pos + k < n) ? s[pos + k] : (u8)0; memcpy(&q, tb, 16); }
  memcpy(tb, &q, 16);
  u32 last = 0;
  if (pos < n) {
    u32 prv = (pos > 0) ? (u32)s[pos - 1] : ((u32)tb[0] ^ 1u);
#pragma unroll
    for (int k = 0; k < 16; k++) { if (pos + k < n && (u32)tb[k] != prv) last = (u32)(pos + k + 1); prv = tb[k]; }
  }
  for (int d = 1; d < 64; d <<= 1) last = max(last, (u32)__shfl_xor((int)last, d, 64));
  if (kz_lane() == 0) wl[threadIdx.x >> 6] = last;
  __syncthreads();
  if (doHist) {                                                        // one LDS add per group of equal bytes among 64 lanes
    const u32 wq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const bool valid = pos + k < n;
      const u32 c = (wq[k >> 2] >> (8 * (k & 3))) & 0xFFu;
      const u64 peers = kz_match8(c, valid);
      if (valid && (peers & kz_lanemask_lt()) == 0) atomicAdd(&h[c], (u32)__popcll(peers));
    }
    __syncthreads();
    const u32 c = h[threadIdx.x];
    if (c) atomicAdd(&S.hist[(int64_t)b * 256 + threadIdx.x], c);
  }
  if (threadIdx.x == 0) { u32 m = 0; for (int w = 0; w < KZ_WG / 64; w++) m = max(m, wl[w]); S.tLastB[(int64_t)b * S.T + t] = m; }
}

// ---- forward scan: per block the reference's preamble (:78-149) and the run start in front of every tile ---------------------
__global__ __launch_bounds__(256) void k_rlt_fscan(const int32_t* __restrict__ d_len, int32_t* __restrict__ d_dtype, RlScratch S, int findBest) {
  const int b = blockIdx.x;
  const int n = d_len[b];
  const int tid = threadIdx.x;
  __shared__ long long lds4[4];
  __shared__ u64 wmin[4];
  int dt = d_dtype[b];
  bool decl = n < 16;                                                                      // :78-79 (0: the caller's)
  if (dt == DT_DNA || dt == DT_BASE64 || dt == DT_UTF8) decl = true;                       // :97-99
  u32 esc = 0xFBu;                                                                         // DEFAULT_ESCAPE :38
  if (findBest && !decl) {                                                                 // :117-149 (uniform)
    const u32 f = S.hist[(int64_t)b * 256 + tid];
    if (dt == DT_UNDEFINED) {
      dt = kz_detect_simple_type_wg(n, (int)f, (int)S.hist[(int64_t)b * 256 + 0x3D], lds4);
      if (tid == 0 && dt != DT_UNDEFINED) d_dtype[b] = dt;                                 // :126-127
      if (dt == DT_DNA || dt == DT_BASE64 || dt == DT_UTF8) decl = true;
    }
    u64 key = ((u64)f << 8) | (u64)tid;                                                    // the lowest symbol of minimal frequency :134-148
    for (int d = 1; d < 64; d <<= 1) { const u64 o = __shfl_xor(key, d, 64); key = o < key ? o : key; }
    __syncthreads();
    if ((tid & 63) == 0) wmin[tid >> 6] = key;
    __syncthreads();
    key = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    esc = (u32)(key & 0xFFu);
  }
  if (tid == 0) { S.esc[b] = (int32_t)esc; S.decl[b] = decl ? 1 : 0; S.fail[b] = 0; S.total[b] = 0; }
  if (decl || tid >= 64) return;
  const int tiles = (n + RL_TILE - 1) / RL_TILE;
  const int64_t o = (int64_t)b * S.T;
  u32 carry = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + tid;
    const u32 lb = (t < tiles) ? S.tLastB[o + t] : 0u;
    const u32 inc = kz_wave_incl_max(lb);
    u32 ex = __shfl_up(inc, 1, 64); if (tid == 0) ex = 0;
    ex = max(ex, carry);
    if (t < tiles) S.tS[o + t] = ex;
    carry = max(carry, (u32)__shfl((int)inc, 63, 64));
  }
}

// ---- forward 1 and 3: one lane per byte ------------------------------------------------------------------------------------------
// per row: the run start of every lane (last boundary at or below it, or the carry), the look-ahead window, the item
#define RL_ROW_BEGIN(r)                                                                                   \
    const u64 m = bnd[r];                                                                                 \
    const int pos = wbase + 64 * (r) + lane;                                                              \
    const u64 le = m & ((2ULL << lane) - 1ULL);                                                           \
    const u32 rs = le ? (u32)(wbase + 64 * (r) + 63 - (int)__builtin_clzll(le)) : carry - 1u;             \
    const u64 win = (m >> lane) | (lane ? (bnd[(r) + 1] << (64 - lane)) : 0ULL);                          \
    const u32 z = (u32)__builtin_ctzll((win >> 1) | (1ULL << 62));                                        \
    const bool act = pos + 6 <= n;
#define RL_ROW_END(r) if (m) carry = (u32)(wbase + 64 * (r) + 64 - (int)__builtin_clzll(m));

__global__ __launch_bounds__(KZ_WG) void k_rlt_f1(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, RlScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RL_TILE;
  if (tstart >= n || S.decl[b]) return;
  const u8* s = src + (int64_t)b * stride;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const int wbase = tstart + wave * (64 * RL_WROWS);
  __shared__ u32 wLast[KZ_WG / 64], wSum[KZ_WG / 64];
  __shared__ __attribute__((aligned(16))) u8 inb[RL_TILE + 32];
  RL_LOAD_ROWS(inb)
  if (lane == 0) wLast[wave] = myLast;
  __syncthreads();
  u32 carry = S.tS[(int64_t)b * S.T + t];                       // position + 1 of the last boundary before the row
  for (int w = 0; w < wave; w++) carry = max(carry, wLast[w]);
  const u32 esc = (u32)S.esc[b];
  u32 sum = 0;
#pragma unroll
  for (int r = 0; r < RL_WROWS; r++) {
    RL_ROW_BEGIN(r)
    if (act) { u32 run; sum += rl_item((u32)pos, (u32)n, rs, v[r], z, esc, &run); }
    if (pos == n - 5) S.s5[b] = rs;
    RL_ROW_END(r)
  }
  const u32 inc = kz_wave_incl_sum(sum);
  if (lane == 63) wSum[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) { u32 tot = 0; for (int w = 0; w < KZ_WG / 64; w++) tot += wSum[w]; S.tSum[(int64_t)b * S.T + t] = tot; }
}

__global__ __launch_bounds__(64) void k_rlt_fsum(const int32_t* __restrict__ d_len, RlScratch S) {
  const int b = blockIdx.x;
  const int n = d_len[b];
  if (S.decl[b]) return;
  const int tiles = (n + RL_TILE - 1) / RL_TILE;
  const int64_t o = (int64_t)b * S.T;
  const int lane = kz_lane();
  u32 carry = 0;                                                 // at most 2 n + 6: fits
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + lane;
    const u32 sz = (t < tiles) ? S.tSum[o + t] : 0u;
    const u32 inc = kz_wave_incl_sum(sz);
    if (t < tiles) S.tOff[o + t] = carry + inc - sz;
    carry += (u32)__shfl((int)inc, 63, 64);
  }
  if (lane == 0) S.total[b] = (int32_t)min(carry, 0x7FFFFFFFu);
}

__global__ __launch_bounds__(KZ_WG) void k_rlt_f3(const u8* __restrict__ src, u8* __restrict__ dst, int64_t stride,
                                                    const int32_t* __restrict__ d_len, RlScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RL_TILE;
  if (tstart >= n || S.decl[b]) return;
  const u8* s = src + (int64_t)b * stride;
  u8* d = dst + (int64_t)b * stride;
  const int wave = threadIdx.x >> 6, lane = kz_lane();
  const int wbase = tstart + wave * (64 * RL_WROWS);
  __shared__ u32 wLast[KZ_WG / 64], wSum[KZ_WG / 64];
  // the tile's output is contiguous: put together in LDS at the output's alignment modulo 16, copied out in 16-byte pieces.
  // At most two bytes per input byte, and a coded piece (6 bytes) stands for at least four: 2 RL_TILE + 6, + 15 of alignment.
  __shared__ __attribute__((aligned(16))) u8 stage[2 * RL_TILE + 64];
  RL_LOAD_ROWS(stage)                                              // (the staging buffer holds the input first)
  if (lane == 0) wLast[wave] = myLast;
  __syncthreads();                                                 // every v[] / bnd[] is in registers: the buffer is free
  u32 carry0 = S.tS[(int64_t)b * S.T + t];
  for (int w = 0; w < wave; w++) carry0 = max(carry0, wLast[w]);
  const u32 esc = (u32)S.esc[b];
  const u32 tileBase = S.tOff[(int64_t)b * S.T + t];
  const u32 base16 = tileBase & ~15u;
  const u32 dstEnd = (u32)(S.dstEnd ? S.dstEnd[b] : S.dstEndAll);
  u32 szv[RL_WROWS], runv[RL_WROWS];
  u32 sum = 0;
  {
    u32 carry = carry0;
#pragma unroll
    for (int r = 0; r < RL_WROWS; r++) {
      RL_ROW_BEGIN(r)
      szv[r] = 0; runv[r] = 0;
      if (act) { szv[r] = rl_item((u32)pos, (u32)n, rs, v[r], z, esc, &runv[r]); sum += szv[r]; }
      RL_ROW_END(r)
    }
  }
  {
    const u32 inc = kz_wave_incl_sum(sum);
    if (lane == 63) wSum[wave] = inc;
  }
  __syncthreads();
  u32 off0 = tileBase, total = 0;
  for (int w = 0; w < KZ_WG / 64; w++) { if (w < wave) off0 += wSum[w]; total += wSum[w]; }
  bool fail = false;
#pragma unroll
  for (int r = 0; r < RL_WROWS; r++) {
    const u32 sz = szv[r];
    if (kz_ballot(sz != 0u) == 0) continue;                        // uniform
    const u32 inc = kz_wave_incl_sum(sz);
    const u32 off = off0 + inc - sz;
    off0 += (u32)__builtin_amdgcn_readlane((int)inc, 63);
    if (sz == 0u) continue;
    const u32 val = v[r];
    u8* o = stage + (off - base16);
    const int pos = wbase + 64 * r + lane;
    if (pos == 0) { o[0] = (u8)esc; o[1] = (u8)val; if (val == esc) o[2] = 0; }        // :154-158
    else if (runv[r]) {                                                                  // :185-197
      if (off + 6u >= dstEnd) fail = true;
      u32 k = 0;
      o[k++] = (u8)val;
      if (val == esc) o[k++] = 0;
      o[k++] = (u8)esc;
      rl_emit_len(o, k, runv[r]);
    } else {                                                                             // :198-216, seen from the piece's last byte
      if (off + sz >= dstEnd) fail = true;
      o[0] = (u8)val;
      if (sz == 2u) o[1] = 0;
    }
  }
  if (fail) atomicOr(&S.fail[b], 1);
  __syncthreads();
  // (an output that reaches n bytes is declined by :262 and its bytes are discarded: nothing is written at or behind n)
  const u32 endLim = min(tileBase + total, (u32)n);
  const bool al = (((uintptr_t)d) & 15) == 0;
  for (u32 g0 = base16 + 16u * threadIdx.x; g0 < endLim; g0 += 16u * KZ_WG) {
    if (al && g0 >= tileBase && g0 + 16 <= endLim) *(uint4*)(d + g0) = *(const uint4*)(stage + (g0 - base16));
    else {
#pragma unroll
      for (int k = 0; k < 16; k++) { const u32 g = g0 + k; if (g >= tileBase && g < endLim) d[g] = stage[g - base16]; }
    }
  }
}

// ---- forward tail: one lane per block.  The piece that holds byte n - 5 in closed form, then RLT.java:218-262 as written ----------
__global__ __launch_bounds__(64) void k_rlt_ftail(const u8* __restrict__ src, u8* __restrict__ dst, int64_t stride, const int32_t* __restrict__ d_len,
                                                  int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag, RlScratch S, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = d_len[b];
  if (n == 0) { d_len2[b] = 0; d_flag[b] = 1; return; }                                  // :70-71
  if (S.decl[b]) { d_len2[b] = n; d_flag[b] = 0; return; }
  const u8* s = src + (int64_t)b * stride;
  u8* d = dst + (int64_t)b * stride;
  const u32 esc = (u32)S.esc[b];
  const int dstEnd = S.dstEnd ? S.dstEnd[b] : S.dstEndAll;
  int dstIdx = S.total[b];
  bool res = (S.fail[b] == 0) && dstIdx < n;                       // n bytes and more: declined by :262 (at most 16 more bytes are written here)
  int srcIdx = n;
  if (res) {
    const u32 p1 = rl_head(S.s5[b], (u32)n - 5u);                  // the head of the piece that holds byte n - 5
    u32 prev = s[p1];
    int run = (p1 == 0u) ? 0 : 1;
    srcIdx = (int)p1 + 1;
    if ((int)p1 < n - 5) {                                         // the loop goes on (:222): the piece ends where a byte differs, at its
      int e = n - 4;                                               // 73 469th counted byte or at the first multiple of four at or behind n - 4 (:178)
      while (e < n && (u32)s[e] == prev) e++;
      const int cut = (int)p1 + (int)((p1 == 0u) ? RL_PIECE0 : RL_PIECE);
      const int e4 = (int)p1 + 1 + 4 * ((n - 5 - (int)p1 + 3) / 4);
      const int q = min(e, min(cut, e4));
      run = q - (int)p1 - ((p1 == 0u) ? 1 : 0);
      srcIdx = q;
      if (run > 3) {                                               // :185-197
        if (dstIdx + 6 >= dstEnd) res = false;
        else {
          d[dstIdx++] = (u8)prev;
          if (prev == esc) d[dstIdx++] = 0;
          d[dstIdx++] = (u8)esc;
          dstIdx = (int)rl_emit_len(d, (u32)dstIdx, (u32)run);
        }
      } else if (prev != esc) {                                    // :198-205
        if (dstIdx + run >= dstEnd) res = false;
        else while (run-- > 0) d[dstIdx++] = (u8)prev;
      } else {                                                     // :206-216
        if (dstIdx + 2 * run >= dstEnd) res = false;
        else while (run-- > 0) { d[dstIdx++] = (u8)esc; d[dstIdx++] = 0; }
      }
      if (res) { prev = s[srcIdx]; srcIdx++; run = 1; }            // :218-220, and :222 leaves the loop
    }
    if (res) {                                                     // :226-260
      if (prev != esc) { if (dstIdx + run < dstEnd) while (run-- > 0) d[dstIdx++] = (u8)prev; }
      else if (dstIdx + 2 * run < dstEnd) while (run-- > 0) { d[dstIdx++] = (u8)esc; d[dstIdx++] = 0; }
      while (srcIdx < n && dstIdx < dstEnd) {
        if ((u32)s[srcIdx] == esc) {
          if (dstIdx + 2 >= dstEnd) { res = false; break; }
          d[dstIdx++] = (u8)esc; d[dstIdx++] = 0; srcIdx++;
          continue;
        }
        d[dstIdx++] = s[srcIdx++];
      }
      res &= (srcIdx == n);                                        // :259
    }
  }
  res &= dstIdx < srcIdx;                                          // :262
  d_len2[b] = res ? dstIdx : n;
  d_flag[b] = res ? 1 : 0;
}

// =================================================================================================
// inverse
#define RI_PER 16
#define RI_TILE (KZ_WG * RI_PER)
#define RI_IDENT (0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12))
// states: 0 a token starts here, 1 behind an escape mark (first length byte), 2 second byte of a two-byte length, 3 / 4 second / third
// byte of a three-byte length.  The map of a byte: entry k (3 bits) = the state behind it when it is read in state k.
__device__ __forceinline__ u32 ri_bytemap(u32 x, u32 esc) {
  const u32 t0 = (x == esc) ? 1u : 0u;                                   // :337, :346
  const u32 t1 = (x == 0xFFu) ? 3u : ((x >= RL_ENC1) ? 2u : 0u);        // :356, :366, :375
  return t0 | (t1 << 3) | (4u << 9);
}
__device__ __forceinline__ u32 ri_compose(u32 a, u32 m) {                // a first, then m
  u32 r = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) r |= ((m >> (3u * ((a >> (3 * k)) & 7u))) & 7u) << (3 * k);
  return r;
}

struct RiScratch {
  u32* tMap;       // [B][T] the tile's transition map
  u32* tState;     // [B][T] state at the tile's start
  u32* tSum;       // [B][T] output bytes of the tokens that END in the tile
  u32* tLit;       // [B][T] 0x100 | value of the tile's last literal / escape literal token, 0: none
  u32* tOff;       // [B][T] exclusive sum of tSum (valid when the total fits)
  u32* tVal;       // [B][T] the last byte produced before the tile (0x100 | value, 0: none)
  int32_t* total;  // [B]
  int32_t* fail;   // [B]
  int32_t* lastEsc;// [B] the input ends with an escape literal token
  int T;
};

// the thread's 16 bytes (identity behind the block's end and for byte 0, the escape itself) -> its map; every thread gets
// the map of the threads before it in the tile (exclusive) and thread 0's caller the tile's
__device__ __forceinline__ u32 ri_thread_map(const u32* wq, int pos, int n, u32 esc) {
  u32 m = RI_IDENT;
#pragma unroll
  for (int k = 0; k < RI_PER; k++) {
    const u32 x = (wq[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    if (pos + k >= 1 && pos + k < n) m = ri_compose(m, ri_bytemap(x, esc));
  }
  return m;
}
__device__ __forceinline__ u32 ri_wg_excl_map(u32 m, u32* lds, u32* tileMap) {
  const int lane = kz_lane(), wave = threadIdx.x >> 6;
  u32 inc = m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if (lane >= d) inc = ri_compose(up, inc); }
  u32 ex = __shfl_up(inc, 1, 64); if (lane == 0) ex = RI_IDENT;
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  u32 pre = RI_IDENT, all = RI_IDENT;
  for (int w = 0; w < KZ_WG / 64; w++) { if (w < wave) pre = ri_compose(pre, lds[w]); all = ri_compose(all, lds[w]); }
  *tileMap = all;
  return ri_compose(pre, ex);
}
__device__ __forceinline__ void ri_load(const u8* s, int pos, int n, u32* wq) {
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (pos + 16 <= n) q = *(const uint4*)(s + pos);
  else if (pos < n) { u8 tb[16]; for (int k = 0; k < 16; k++) tb[k] = (pos + k < n) ? s[pos + k] : (u8)0; memcpy(&q, tb, 16); }
  wq[0] = q.x; wq[1] = q.y; wq[2] = q.z; wq[3] = q.w;
}

__global__ __launch_bounds__(KZ_WG) void k_rlt_i1(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, RiScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RI_TILE;
  if (tstart >= n) return;
  __shared__ u32 lds[KZ_WG / 64];
  const u8* s = src + (int64_t)b * stride;
  const int pos = tstart + (int)threadIdx.x * RI_PER;
  u32 wq[4];
  ri_load(s, pos, n, wq);
  u32 tileMap;
  (void)ri_wg_excl_map(ri_thread_map(wq, pos, n, (u32)s[0]), lds, &tileMap);
  if (threadIdx.x == 0) S.tMap[(int64_t)b * S.T + t] = tileMap;
}

__global__ __launch_bounds__(64) void k_rlt_iscan(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, RiScratch S) {
  const int b = blockIdx.x;
  const int n = d_len[b];
  const int lane = kz_lane();
  const int tiles = (n + RI_TILE - 1) / RI_TILE;
  const int64_t o = (int64_t)b * S.T;
  u32 state = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + lane;
    u32 inc = (t < tiles) ? S.tMap[o + t] : RI_IDENT;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if (lane >= d) inc = ri_compose(up, inc); }
    u32 ex = __shfl_up(inc, 1, 64); if (lane == 0) ex = RI_IDENT;
    if (t < tiles) S.tState[o + t] = (ex >> (3u * state)) & 7u;
    const u32 all = (u32)__shfl((int)inc, 63, 64);
    state = (all >> (3u * state)) & 7u;
  }
  if (lane == 0) {
    const u8* s = src + (int64_t)b * stride;
    bool fail = false;
    if (n > 0) {
      if (n < 2) fail = true;                                      // (the reference reads src[1] here: outside the block)
      else if (state != 0u) fail = true;                           // an escape mark or an unfinished length at the end :348-351, :366-379
      else if (n > 2 && s[1] == s[0] && s[2] != 0) fail = true;    // the data cannot start with a run :324-329
    }
    S.fail[b] = fail ? 1 : 0; S.total[b] = 0; S.lastEsc[b] = 0;
  }
}

// One step of the reference's loop (:336-404) on byte x in state st: returns the output bytes of the token that ends here (0: none)
// and *kind: 1 literal, 2 escape literal, 3 run.  acc holds the length bytes read so far.
__device__ __forceinline__ u32 ri_step(u32 x, u32 esc, u32& st, u32& acc, int* kind) {
  *kind = 0;
  switch (st) {
    case 0: if (x != esc) { *kind = 1; return 1u; } st = 1; return 0u;
    case 1:
      if (x == 0u) { st = 0; *kind = 2; return 1u; }                                       // :356-363
      if (x == 0xFFu) { st = 3; return 0u; }
      if (x >= RL_ENC1) { st = 2; acc = x - RL_ENC1; return 0u; }
      st = 0; *kind = 3; return x + 2u;                                                    // :385
    case 2: st = 0; *kind = 3; return ((acc << 8) | x) + RL_ENC1 + 2u;                     // :381-385
    case 3: st = 4; acc = x; return 0u;
    default: st = 0; *kind = 3; return ((acc << 8) | x) + RL_ENC2 + 2u;                    // :372-374, :385 (at most MAX_RUN: :387's second test never holds)
  }
}
// state and length bytes a thread starts with
#define RI_ENTER()                                                                                        \
  u32 wq[4];                                                                                              \
  ri_load(s, pos, n, wq);                                                                                 \
  u32 tileMap;                                                                                            \
  const u32 exm = ri_wg_excl_map(ri_thread_map(wq, pos, n, esc), ldsm, &tileMap);                         \
  u32 st = (exm >> (3u * S.tState[(int64_t)b * S.T + t])) & 7u;                                           \
  u32 acc = 0;                                                                                            \
  if (pos < n) { if (st == 2u) acc = (u32)s[pos - 1] - RL_ENC1; else if (st == 4u) acc = (u32)s[pos - 1]; }

__global__ __launch_bounds__(KZ_WG) void k_rlt_i2(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, RiScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RI_TILE;
  if (tstart >= n || S.fail[b]) return;
  __shared__ u32 ldsm[KZ_WG / 64];
  __shared__ u32 lds[32];
  const u8* s = src + (int64_t)b * stride;
  const int pos = tstart + (int)threadIdx.x * RI_PER;
  const u32 esc = (u32)s[0];
  RI_ENTER()
  u32 sum = 0, lit = 0;
#pragma unroll
  for (int k = 0; k < RI_PER; k++) {
    const int i = pos + k;
    if (i < 1 || i >= n) continue;
    const u32 x = (wq[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    int kind;
    sum += ri_step(x, esc, st, acc, &kind);
    if (kind == 1) lit = 0x100u | x; else if (kind == 2) lit = 0x100u | esc;
    if (i == n - 1 && kind == 2) S.lastEsc[b] = 1;
  }
  u32 total;
  (void)kz_wg_excl_sum(sum, lds, &total);
  u32 mx;
  (void)kz_wg_incl_max(lit ? (((u32)threadIdx.x + 1u) << 9) | lit : 0u, lds, &mx);
  if (threadIdx.x == 0) { S.tSum[(int64_t)b * S.T + t] = total; S.tLit[(int64_t)b * S.T + t] = mx & 0x1FFu; }
}

__global__ __launch_bounds__(64) void k_rlt_isum(const int32_t* __restrict__ d_len, RiScratch S, int dstCap) {
  const int b = blockIdx.x;
  const int n = d_len[b];
  if (S.fail[b]) return;
  const int tiles = (n + RI_TILE - 1) / RI_TILE;
  const int64_t o = (int64_t)b * S.T;
  const int lane = kz_lane();
  u64 carry = 0;
  u32 carryVal = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + lane;
    const u32 v = (t < tiles) ? S.tSum[o + t] : 0u;
    u64 inc = v;
    for (int d = 1; d < 64; d <<= 1) { const u64 up = __shfl_up(inc, d, 64); if (lane >= d) inc += up; }
    if (t < tiles) S.tOff[o + t] = (u32)(carry + inc - v);
    carry += __shfl(inc, 63, 64);
    const u32 lt = (t < tiles) ? S.tLit[o + t] : 0u;
    const u32 mi = kz_wave_incl_max(lt ? (((u32)lane + 1u) << 9) | lt : 0u);
    u32 ex = __shfl_up(mi, 1, 64); if (lane == 0) ex = 0;
    if (t < tiles) S.tVal[o + t] = ex ? (ex & 0x1FFu) : carryVal;
    const u32 last = (u32)__shfl((int)mi, 63, 64);
    if (last) carryVal = last & 0x1FFu;
  }
  if (lane == 0) {
    // a literal or a run that does not fit fails (:339-340 with :406, :387); an escape literal that does not fit leaves the loop with its
    // two bytes read (:358-359): when it is the last token the input is used up and the block succeeds without that byte
    if (carry <= (u64)dstCap) S.total[b] = (int32_t)carry;
    else if (carry == (u64)dstCap + 1u && S.lastEsc[b]) S.total[b] = dstCap;
    else { S.fail[b] = 1; S.total[b] = 0; }
  }
}

// `len` bytes `val` at d + o, by all lanes of the wave
__device__ __forceinline__ void ri_fill(u8* d, u32 o, u32 len, u32 val, int lane) {
  u8* p = d + o;
  const u32 head = min(len, (u32)((16u - (u32)((uintptr_t)p & 15u)) & 15u));
  if ((u32)lane < head) p[lane] = (u8)val;
  const u32 body = (len - head) >> 4;
  const u32 w4 = val * 0x01010101u;
  const uint4 q = make_uint4(w4, w4, w4, w4);
  uint4* p16 = (uint4*)(p + head);
  for (u32 j = (u32)lane; j < body; j += 64u) p16[j] = q;
  const u32 done = head + (body << 4);
  if ((u32)lane < len - done) p[done + lane] = (u8)val;
}

__global__ __launch_bounds__(KZ_WG) void k_rlt_i3(const u8* __restrict__ src, u8* __restrict__ dst, int64_t stride,
                                                    const int32_t* __restrict__ d_len, RiScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = d_len[b];
  const int tstart = t * RI_TILE;
  if (tstart >= n || S.fail[b]) return;
  __shared__ u32 ldsm[KZ_WG / 64];
  __shared__ u32 lds[32];
  const u8* s = src + (int64_t)b * stride;
  u8* d = dst + (int64_t)b * stride;
  const int pos = tstart + (int)threadIdx.x * RI_PER;
  const int lane = kz_lane();
  const u32 esc = (u32)s[0];
  const u32 cap = (u32)S.total[b];                                  // nothing is written at or behind the block's decoded length
  RI_ENTER()
  const u32 st0 = st, acc0 = acc;
  u32 sum = 0, lit = 0;
#pragma unroll
  for (int k = 0; k < RI_PER; k++) {
    const int i = pos + k;
    if (i < 1 || i >= n) continue;
    const u32 x = (wq[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    int kind;
    sum += ri_step(x, esc, st, acc, &kind);
    if (kind == 1) lit = 0x100u | x; else if (kind == 2) lit = 0x100u | esc;
  }
  u32 total;
  u32 off = kz_wg_excl_sum(sum, lds, &total) + S.tOff[(int64_t)b * S.T + t];
  u32 mx;
  const u32 key = lit ? (((u32)threadIdx.x + 1u) << 9) | lit : 0u;
  const u32 incm = kz_wg_incl_max(key, lds, &mx);
  // the last byte produced before this thread: the inclusive maximum of the thread before it, else the tile's carry
  u32 exm2 = __shfl_up(incm, 1, 64);
  __syncthreads();
  if (lane == 63) lds[20 + (threadIdx.x >> 6)] = incm;
  __syncthreads();
  if (lane == 0) exm2 = (threadIdx.x >= 64) ? lds[20 + (threadIdx.x >> 6) - 1] : 0u;
  u32 lastVal = exm2 ? (exm2 & 0xFFu) : (S.tVal[(int64_t)b * S.T + t] & 0xFFu);
  st = st0; acc = acc0;
  for (int k = 0; k < RI_PER; k++) {                                 // in step: the long runs of the wave's lanes are written by all of them
    const int i = pos + k;
    const u32 x = (wq[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    int kind = 0;
    u32 sz = 0;
    if (i >= 1 && i < n) sz = ri_step(x, esc, st, acc, &kind);
    const u32 at = off;
    off += sz;
    if (kind == 1) { if (at < cap) d[at] = (u8)x; lastVal = x; }
    else if (kind == 2) { if (at < cap) d[at] = (u8)esc; lastVal = esc; }
    const bool isLong = (kind == 3) && sz >= 32u;
    if (kind == 3 && !isLong) for (u32 j = 0; j < sz; j++) d[at + j] = (u8)lastVal;
    u64 m = kz_ballot(isLong);
    while (m) {
      const int l = (int)__builtin_ctzll(m);
      m &= m - 1ULL;
      ri_fill(d, (u32)__shfl((int)at, l, 64), (u32)__shfl((int)sz, l, 64), (u32)__shfl((int)lastVal, l, 64), lane);
    }
  }
}

__global__ void k_rlt_ifin(const int32_t* __restrict__ d_len, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag, RiScratch S, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool fail = S.fail[b] != 0;
  d_len2[b] = fail ? 0 : ((d_len[b] == 0) ? 0 : S.total[b]);
  d_flag[b] = fail ? 0 : 1;
}

// =================================================================================================
size_t kz_rlt_scratch(int B, int maxN) {
  const int T = (maxN + RL_TILE - 1) / RL_TILE + 1;
  return (size_t)B * (kz_align((size_t)T * 4, 256) * 6 + 1024 + 256 * 8) + 8192;
}

int kz_stage_rlt_forward(kz_ctx* ctx, kz_batch& bt, int entropy) {
  const int B = bt.B;
  int maxN = 0;
  for (int b = 0; b < B; b++) if (bt.h_len[b] > maxN) maxN = bt.h_len[b];
  // the escape is searched, and the block's type looked at, under every coder but these (:101-108)
  const int findBest = !kz_fast_coder(entropy);
  RlScratch S;
  S.T = (maxN + RL_TILE - 1) / RL_TILE + 1;
  S.tLastB = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tS = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tSum = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tOff = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.hist = (u32*)kz_arena_alloc(ctx, (size_t)B * 256 * 4);
  S.s5 = (u32*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.esc = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.decl = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.fail = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.total = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.dstEnd = bt.d_rltEnd;
  S.dstEndAll = bt.rltEndAll;
  if (!S.total) { snprintf(ctx->err, sizeof(ctx->err), "rlt_forward: arena overflow"); return -KZ_ERR_DEVICE; }
  if (!S.dstEnd && S.dstEndAll <= 0) { snprintf(ctx->err, sizeof(ctx->err), "rlt_forward: no output array length given"); return -KZ_ERR_INVALID_PARAM; }
  hipStream_t st = ctx->stream;
  const u8* src = bt.buf[bt.cur];
  u8* dst = bt.buf[bt.cur ^ 1];
  if (findBest) KZ_HIP(hipMemsetAsync(S.hist, 0, (size_t)B * 256 * 4, st));
  KZ_HIP(hipMemsetAsync(S.s5, 0, (size_t)B * 4, st));
  const int tiles = (maxN + RL_TILE - 1) / RL_TILE;
  if (maxN > 0) KZ_LAUNCH(ctx, KID_RLT_F0, k_rlt_f0, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, bt.d_len, S, findBest);
  KZ_LAUNCH(ctx, KID_RLT_FSCAN, k_rlt_fscan, dim3(B), dim3(256), bt.d_len, bt.d_dtype, S, findBest);
  if (maxN > 0) {
    KZ_LAUNCH(ctx, KID_RLT_F1, k_rlt_f1, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, bt.d_len, S);
    KZ_LAUNCH(ctx, KID_RLT_FSUM, k_rlt_fsum, dim3(B), dim3(64), bt.d_len, S);
    KZ_LAUNCH(ctx, KID_RLT_F3, k_rlt_f3, dim3(tiles, B), dim3(KZ_WG), src, dst, bt.stride, bt.d_len, S);
  }
  KZ_LAUNCH(ctx, KID_RLT_FTAIL, k_rlt_ftail, dim3((B + 63) / 64), dim3(64), src, dst, bt.stride, bt.d_len, bt.d_len2, bt.d_flag, S, B);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}

int kz_stage_rlt_inverse(kz_ctx* ctx, kz_batch& bt, int dstCap) {
  const int B = bt.B;
  int maxN = 0;
  for (int b = 0; b < B; b++) if (bt.h_len[b] > maxN) maxN = bt.h_len[b];
  RiScratch S;
  S.T = (maxN + RI_TILE - 1) / RI_TILE + 1;
  S.tMap = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tState = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tSum = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tLit = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tOff = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tVal = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.total = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.fail = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.lastEsc = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  if (!S.lastEsc) { snprintf(ctx->err, sizeof(ctx->err), "rlt_inverse: arena overflow"); return -KZ_ERR_DEVICE; }
  const u8* src = bt.buf[bt.cur];
  u8* dst = bt.buf[bt.cur ^ 1];
  if ((int64_t)dstCap > bt.stride) dstCap = (int)bt.stride;
  const int tiles = (maxN + RI_TILE - 1) / RI_TILE;
  if (maxN > 0) KZ_LAUNCH(ctx, KID_RLT_I1, k_rlt_i1, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, bt.d_len, S);
  KZ_LAUNCH(ctx, KID_RLT_ISCAN, k_rlt_iscan, dim3(B), dim3(64), src, bt.stride, bt.d_len, S);
  if (maxN > 0) {
    KZ_LAUNCH(ctx, KID_RLT_I2, k_rlt_i2, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, bt.d_len, S);
    KZ_LAUNCH(ctx, KID_RLT_ISUM, k_rlt_isum, dim3(B), dim3(64), bt.d_len, S, dstCap);
    KZ_LAUNCH(ctx, KID_RLT_I3, k_rlt_i3, dim3(tiles, B), dim3(KZ_WG), src, dst, bt.stride, bt.d_len, S);
  }
  KZ_LAUNCH(ctx, KID_RLT_IFIN, k_rlt_ifin, dim3((B + 255) / 256), dim3(256), bt.d_len, bt.d_len2, bt.d_flag, S, B);
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
