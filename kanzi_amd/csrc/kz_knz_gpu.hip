// kz_knz_gpu.hip -- the .knz container on device memory: the bit-granular concatenation of block streams
// (K/io/CompressedOutputStream.java:1024-1035) as a copy kernel, its inverse, and the serial walk of the block length
// prefixes (K/io/CompressedInputStream.java:1127-1129), and the check of a caller's index entries that stands in for the walk in
// the indexed reads; behind them the same steps for many streams in one launch (a table entry per segment, slot or row, each with
// its own bounds: kz_compress_many_device / kz_decompress_many_device), and the splice: the pack over pieces whose payload bits lie
// where they are in their source streams, with the check of every piece against its own source in front of it (kz_knz_splice_device);
// and the copy of the byte-addressed reads: many (range x block) segments of decoded rows to their places in one launch (k_knz_read),
// with its mirror image for the byte-addressed writes: segments of new bytes into decoded rows (k_knz_write).
// For the byte-addressed read of many streams (kz_read_bytes_many_device) the check of index entries has a form over rows of many
// streams that also brings the block-header words (k_knz_check_rows); for the byte-addressed write of many streams
// (kz_write_bytes_many_device) the splice's copy has a form that writes a bit range in each of many slots (k_knz_splice_many).
// Last, the scan (kz_knz_scan_device): the reader's acceptance test at every bit position of a stream and the link step over the
// accepted positions (k_knz_scan_*), which finds a stream's blocks without the walk and behind damage.
// The callers (kz_stream_device.hip: kz_compress_device / kz_decompress_device / kz_decompress_range_device / kz_decode_indexed_device /
// kz_knz_assemble_device / kz_knz_index_device, the two many-stream calls, kz_knz_splice_device, kz_read_bytes_device and
// kz_write_bytes_device) do the bit-offset arithmetic, the stream header and the block-header prechecks on the host; no payload byte
// leaves the device.
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_knz_host.h"
#include <algorithm>

typedef uint8_t u8;
typedef uint32_t u32;
typedef unsigned long long u64;

namespace {
// 16 bytes of the bit string that starts `sh` bits (0..7) into *p, from aligned 32-bit loads: reads the aligned words that cover
// p[0 .. 16] (p[0 .. 15] when the total shift is 0), so the caller makes sure that [p & ~3, (p & ~3) + knz_window(p, sh)) is readable
__device__ __forceinline__ int knz_window(const u8* p, int sh) { return ((((uintptr_t)p & 3) << 3) + sh) ? 20 : 16; }
__device__ __forceinline__ uint4 knz_load128(const u8* p, int sh) {
  const int s = (int)(((uintptr_t)p & 3) << 3) + sh;                    // 0 .. 31
  const u32* a = (const u32*)((uintptr_t)p & ~(uintptr_t)3);
  u32 w[5];
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = __builtin_bswap32(a[i]);
  w[4] = s ? __builtin_bswap32(a[4]) : 0u;
  u32 o[4];
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = s ? ((w[i] << s) | (w[i + 1] >> (32 - s))) : w[i];
  return make_uint4(__builtin_bswap32(o[0]), __builtin_bswap32(o[1]), __builtin_bswap32(o[2]), __builtin_bswap32(o[3]));
}
__device__ __forceinline__ int knz_lw(int64_t W) { return W < 8 ? 3 : kz_ilog2((u32)(W >> 3)) + 4; }   // the device form of knz_prefix_width (kz_knz_host.h)

// ---- the pack's steps, shared by k_knz_pack, k_knz_pack_many and k_knz_splice ----
// Where a field's payload bits lie: bit k of the payload is bit bit0 + k of base[0 .. lim), and base[0 .. lim) is all that may be
// read for it.  A packed block's are the bytes of its row's W bits, a spliced piece's lie anywhere in its source's own segment.
struct KnzPay { const u8* base; int64_t bit0, lim; };
__device__ __forceinline__ KnzPay knz_payload(const u8* __restrict__ rows, const KnzBlk& b) { return KnzPay{rows + b.src, 0, (b.bits + 7) >> 3}; }
__device__ __forceinline__ KnzPay knz_payload(const u8* __restrict__ src, const KnzPiece& b) { return KnzPay{src + b.seg, b.off, b.n}; }
// the last block whose prefix starts at or before pos0 (prefix starts grow with i)
template <class T> __device__ __forceinline__ int knz_find_field(const T* __restrict__ blk, int nb, int64_t pos0) {
  int a = 0, b = nb;                                                                // invariant: prefix start of blocks < a is <= pos0
  while (a < b) {
    const int m = (a + b) >> 1;
    const int64_t W = blk[m].bits;
    if (blk[m].pay - 5 - knz_lw(W) <= pos0) a = m + 1; else b = m;
  }
  return a > 0 ? a - 1 : 0;
}
// the same among the blocks lo .. hi, for a pos0 whose answer is known to lie there
template <class T> __device__ __forceinline__ int knz_find_between(const T* __restrict__ blk, int lo, int hi, int64_t pos0) {
  int a = lo + 1, b = hi + 1;                                                       // invariant: prefix start of block a - 1 is <= pos0
  while (a < b) {
    const int m = (a + b) >> 1;
    if (blk[m].pay - 5 - knz_lw(blk[m].bits) <= pos0) a = m + 1; else b = m;
  }
  return a - 1;
}
__device__ __forceinline__ int64_t knz_first_lane(int64_t v) {                      // v of the wave's first active lane, wave-uniform
  return (int64_t)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)v));
}
// the 16 bytes [pos0, hiBit) of the destination when they lie inside the payload of block j alone: wide load, wide store at `out`.
// From the row only aligned words inside the bytes of its W bits are read (of a piece: inside its source's segment); false, nothing
// stored, when the unit is not of that kind.
template <class T> __device__ __forceinline__ bool knz_wide_unit(const u8* __restrict__ rows, const T* __restrict__ blk, int nb, int j, int64_t pos0, int64_t hiBit, u8* out) {
  if (j >= nb) return false;
  const int64_t pay = blk[j].pay, W = blk[j].bits;
  if (pos0 < pay || hiBit > pay + W) return false;
  const KnzPay y = knz_payload(rows, blk[j]);
  const int64_t k = y.bit0 + (pos0 - pay);
  const u8* p = y.base + (k >> 3);
  const u8* al = (const u8*)((uintptr_t)p & ~(uintptr_t)3);
  if (al < y.base || al + knz_window(p, (int)(k & 7)) > y.base + y.lim) return false;
  *(uint4*)out = knz_load128(p, (int)(k & 7));
  return true;
}
// the byte that ends at bit bend, composed from bit pos on (acc: the bits in front of pos, already in place) out of whatever fields
// it holds; j moves to the last field looked at.  Of a payload only the bytes that hold its W bits are read.
template <class T> __device__ __forceinline__ u8 knz_compose_byte(const u8* __restrict__ rows, const T* __restrict__ blk, int nb, int& j, int64_t pos, int64_t bend, u32 acc) {
  while (pos < bend) {
    while (j < nb && pos >= blk[j].pay + blk[j].bits) j++;
    if (j >= nb) break;                                                             // behind the last field: zeros
    const int64_t pay = blk[j].pay, W = blk[j].bits;
    const int room = (int)(bend - pos);
    u32 v; int take;
    if (pos < pay) {                                                                // length prefix: 5 + lw bits
      const int lw = knz_lw(W), pw = 5 + lw;
      const u64 field = ((u64)(lw - 3) << lw) | (u64)W;
      const int k = (int)(pos - (pay - pw));
      take = (int)(pay - pos) < room ? (int)(pay - pos) : room;
      v = (u32)(field >> (pw - k - take)) & ((1u << take) - 1);
    } else {
      const KnzPay y = knz_payload(rows, blk[j]);
      const int64_t k = pos - pay, sk = y.bit0 + k;
      const int so = (int)(sk & 7);
      take = (W - k) < room ? (int)(W - k) : room;
      const u8* s = y.base + (sk >> 3);
      const u32 two = ((u32)s[0] << 8) | (so + take > 8 ? (u32)s[1] : 0u);
      v = (two >> (16 - so - take)) & ((1u << take) - 1);
    }
    acc |= v << (room - take);
    pos += take;
  }
  return (u8)acc;
}
}  // namespace

// ---- pack: blocks -> container --------------------------------------------------------------------------------------------
// The launch owns the bits [startBit, endBit) of dst: the fields of blk[0 .. nb) back to back from startBit (5 bits lw - 3, lw bits
// W, W payload bits from rows + blk[i].src), then zeros up to endBit (the end marker, :491-492) and to the end of the last byte.
// Output-centric: a lane owns the (at most) 16 bytes of one 16-byte aligned unit of dst and composes them from whatever fields
// they hold, so every byte has one writer and nothing depends on what dst held -- with one exception: when startBit is not on a
// byte boundary, the high bits of the first byte are the previous launch's (same stream), which wrote that byte whole with its
// spare bits zero; they are read back and kept.  From a row only the bytes of its W bits are read.
__global__ void __launch_bounds__(256) k_knz_pack(const u8* __restrict__ rows, const KnzBlk* __restrict__ blk, int nb, u8* dst, int64_t startBit, int64_t endBit) {
  const int64_t firstByte = startBit >> 3, lastByte = (endBit + 7) >> 3;           // [firstByte, lastByte) is written
  const uintptr_t A0 = (uintptr_t)(dst + firstByte) & ~(uintptr_t)15;
  const int64_t units = (int64_t)(((uintptr_t)(dst + lastByte) - A0 + 15) >> 4);
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ub = (int64_t)(A0 - (uintptr_t)dst) + (u << 4);                   // the unit's first byte as an index into dst (may be < firstByte)
    const int64_t lo = ub < firstByte ? firstByte : ub, hi = ub + 16 > lastByte ? lastByte : ub + 16;
    if (lo >= hi) continue;
    const int64_t pos0 = (lo == firstByte) ? startBit : (lo << 3);
    int j = knz_find_field(blk, nb, pos0);
    if (hi - lo == 16 && knz_wide_unit(rows, blk, nb, j, pos0, hi << 3, dst + lo)) continue;
    int64_t pos = pos0;
    for (int64_t b = lo; b < hi; b++) {
      const int64_t bend = (b + 1) << 3;
      const u32 acc = (pos & 7) ? dst[b] & (0xFFu << (8 - (int)(pos & 7))) : 0u;    // only the launch's first byte: see above
      dst[b] = knz_compose_byte(rows, blk, nb, j, pos, bend, acc);
      pos = bend;
    }
  }
}

// ---- splice: blocks of existing streams -> container, bit to bit ----------------------------------------------------------------
// k_knz_pack's launch over pieces whose payloads lie where they are in their sources: piece i is the pc[i].bits bits from bit
// pc[i].off of the stream src[pc[i].seg .. + pc[i].n), at any of the 8 x 8 bit phases of the two sides.  No staging rows: a payload
// bit is loaded once, from its source, and stored once.  A unit wholly inside one payload is one wide store of aligned 32-bit loads
// that stay inside the piece's own source segment; units with a prefix or a payload's end in them, and those whose load window
// would leave the segment, are composed bytewise.  The first byte's high bits are kept as in k_knz_pack.  The caller has checked
// every piece (k_knz_check_many): [off, off + bits) lies inside its segment.
// The field search is what a lane of the pack waits for longest (a dozen dependent loads from the table), and the 64 units of a wave
// lie side by side: the wave searches once for its first and once for its last unit, with wave-uniform arguments, and a lane then
// only among the pieces between the two, as a rule one or two.
__global__ void __launch_bounds__(256) k_knz_splice(const u8* __restrict__ src, const KnzPiece* __restrict__ pc, int np, u8* dst, int64_t startBit, int64_t endBit) {
  const int64_t firstByte = startBit >> 3, lastByte = (endBit + 7) >> 3;           // [firstByte, lastByte) is written
  const uintptr_t A0 = (uintptr_t)(dst + firstByte) & ~(uintptr_t)15;
  const int64_t units = (int64_t)(((uintptr_t)(dst + lastByte) - A0 + 15) >> 4);
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ub = (int64_t)(A0 - (uintptr_t)dst) + (u << 4);                   // the unit's first byte as an index into dst (may be < firstByte)
    const int64_t lo = ub < firstByte ? firstByte : ub, hi = ub + 16 > lastByte ? lastByte : ub + 16;
    if (lo >= hi) continue;
    const int64_t pos0 = (lo == firstByte) ? startBit : (lo << 3);
    const int64_t ub0 = knz_first_lane(ub);                                         // the wave's units: 64 in a row from its first lane's
    const int jlo = knz_find_field(pc, np, ub0 < firstByte ? startBit : (ub0 << 3));
    const int jhi = knz_find_field(pc, np, (ub0 + 63 * 16) << 3);
    int j = knz_find_between(pc, jlo, jhi, pos0);
    if (hi - lo == 16 && knz_wide_unit(src, pc, np, j, pos0, hi << 3, dst + lo)) continue;
    int64_t pos = pos0;
    for (int64_t b = lo; b < hi; b++) {
      const int64_t bend = (b + 1) << 3;
      const u32 acc = (pos & 7) ? dst[b] & (0xFFu << (8 - (int)(pos & 7))) : 0u;    // only the launch's first byte
      dst[b] = knz_compose_byte(src, pc, np, j, pos, bend, acc);
      pos = bend;
    }
  }
}

// ---- walk: the length prefixes, one after the other ---------------------------------------------------------------------------
// One lane (the chain is serial by the format).  From bit `startBit` of src[0 .. n): per block the payload's bit offset, its W, and
// the first 8 bytes of the payload, left aligned (zeros where the stream ends): the block-header bytes the host prechecks.
// res[0] = blocks recorded whole, res[1] = bit position of the next prefix, res[2] = why it stopped: KNZ_WALK_COUNT, _END (the end
// marker, W = 0; res[1] is behind it), _PREFIX (a prefix does not fit in 8 n bits; res[1] is that prefix) or _PAYLOAD (a payload
// does not fit: its entry is recorded at index res[0] all the same, res[1] is its payload).  Nothing outside src[0 .. n) is read.
__device__ __forceinline__ u64 knz_peek64(const u8* __restrict__ src, int64_t n, int64_t pos) {   // 57 bits or more from bit pos, left aligned
  const int64_t by = pos >> 3;
  u64 hi = 0; u32 lo = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) hi = (hi << 8) | (by + i < n ? (u64)src[by + i] : 0ull);
  lo = by + 8 < n ? (u32)src[by + 8] : 0u;
  const int sh = (int)(pos & 7);
  return sh ? ((hi << sh) | (lo >> (8 - sh))) : hi;
}
// the walk of one stream p[0 .. n) by one lane: entry i goes to index base + i of off / bits / hdr when i < cap, res[0 .. 3) as above
// (base by value, not folded into the pointers: the tables' addresses stay wave-uniform)
__device__ __forceinline__ void knz_walk_stream(const u8* __restrict__ p, int64_t n, int64_t startBit, int maxCount, int cap, int64_t base,
                                                int64_t* __restrict__ off, int64_t* __restrict__ bits, u64* __restrict__ hdr, int64_t* __restrict__ res) {
  const int64_t nbits = n << 3;
  int64_t pos = startBit;
  int cnt = 0, why = KNZ_WALK_COUNT;
  while (cnt < maxCount) {
    if (pos + 5 > nbits) { why = KNZ_WALK_PREFIX; break; }
    const u64 w = knz_peek64(p, n, pos);                                            // 5 + 34 bits at the most
    const int lr = (int)(w >> 59) + 3;
    if (pos + 5 + lr > nbits) { why = KNZ_WALK_PREFIX; break; }
    const int64_t W = (int64_t)((w << 5) >> (64 - lr));
    const int64_t pay = pos + 5 + lr;
    if (W == 0) { why = KNZ_WALK_END; pos = pay; break; }
    if (cnt < cap) { off[base + cnt] = pay; bits[base + cnt] = W; hdr[base + cnt] = knz_peek64(p, n, pay); }   // (bytes at and behind p[n] read as zero)
    pos = pay;
    if (W > nbits - pay) { why = KNZ_WALK_PAYLOAD; break; }
    pos = pay + W;
    cnt++;
  }
  res[0] = cnt; res[1] = pos; res[2] = why;
}
__global__ void k_knz_walk(const u8* __restrict__ src, int64_t n, int64_t startBit, int maxCount,
                           int64_t* __restrict__ off, int64_t* __restrict__ bits, u64* __restrict__ hdr, int64_t* __restrict__ res) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  knz_walk_stream(src, n, startBit, maxCount, maxCount, 0, off, bits, hdr, res);   // cap = maxCount: every entry is recorded, the one of a payload that does not fit included
}

// ---- check: index entries against the stream, each on its own ------------------------------------------------------------------
// One lane per entry (off[i], bits[i]) of a caller's index.  bad[i] = 0 if the walk could have recorded the entry at this place:
// W = bits[i] > 0, the payload [off, off + W) inside the 8 n bits of src, and for some lr in 3 .. 34 the 5 + lr bits in front of off
// lie at or behind bit hdrEnd (the end of the stream header) and read (lr - 3, W); else 1.  hdr[i] = the payload's first 8 bytes,
// left aligned, as the walk gives them (0 for a bad entry).  That makes k_knz_unpack and the decoders safe on the entry; it does
// not prove that the entry lies on the chain of prefixes from hdrEnd.  Nothing outside src[0 .. n) is read: hdrEnd >= 160, so the
// 39 bits in front of a good off start inside src, and knz_peek64 reads bytes at and behind src[n] as zero.
__device__ __forceinline__ bool knz_entry_ok(const u8* __restrict__ src, int64_t n, int64_t hdrEnd, int64_t o, int64_t W) {
  const int64_t nbits = n << 3;
  if (!(W > 0 && W < (1ll << 34) && o >= hdrEnd + 8 && o >= 39 && o <= nbits && W <= nbits - o)) return false;
  const u64 x = knz_peek64(src, n, o - 39) >> 25;                                     // the 39 bits in front of o
  for (int lr = 64 - __clzll((long long)W) < 3 ? 3 : 64 - __clzll((long long)W); lr <= 34; lr++) {
    if (o - 5 - lr < hdrEnd) break;
    const u64 f = x & ((1ull << (5 + lr)) - 1);
    if ((int)(f >> lr) + 3 == lr && (int64_t)(f & ((1ull << lr) - 1)) == W) return true;
  }
  return false;
}
__global__ void __launch_bounds__(256) k_knz_check(const u8* __restrict__ src, int64_t n, int64_t hdrEnd, const int64_t* __restrict__ off,
                                                   const int64_t* __restrict__ bits, int nb, u64* __restrict__ hdr, int64_t* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const bool ok = knz_entry_ok(src, n, hdrEnd, off[i], bits[i]);
  hdr[i] = ok ? knz_peek64(src, n, off[i]) : 0;
  bad[i] = ok ? 0 : 1;
}
// the same rule for the pieces of a splice, each against its own source: the stream src[pc[i].seg .. + pc[i].n), whose header ends at
// bit pc[i].hdrEnd.  bad[i] = 0 / 1.  Nothing outside that segment is read, not even a neighbour's bytes in the same buffer.
__global__ void __launch_bounds__(256) k_knz_check_many(const u8* __restrict__ src, const KnzPiece* __restrict__ pc, int np, int32_t* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  bad[i] = knz_entry_ok(src + pc[i].seg, pc[i].n, pc[i].hdrEnd, pc[i].off, pc[i].bits) ? 0 : 1;
}
// both at once for the index entries of many streams (kz_read_bytes_many_device): entry i is (t[i].off, t[i].bits) against its own
// stream src[t[i].seg .. + t[i].n), whose header ends at bit t[i].hdrEnd.  bad[i] = 0 / 1 by the same rule, hdr[i] = the payload's
// first 8 bytes, left aligned, as k_knz_check gives them (0 for a bad entry).  Nothing outside that segment is read.
__global__ void __launch_bounds__(256) k_knz_check_rows(const u8* __restrict__ src, const KnzCheckRow* __restrict__ t, int nr, u64* __restrict__ hdr, int64_t* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nr) return;
  const KnzCheckRow r = t[i];
  const u8* s = src + r.seg;
  const bool ok = knz_entry_ok(s, r.n, r.hdrEnd, r.off, r.bits);
  hdr[i] = ok ? knz_peek64(s, r.n, r.off) : 0;
  bad[i] = ok ? 0 : 1;
}

// ---- unpack: container -> byte-aligned rows ------------------------------------------------------------------------------------
// Row i (rows + i * stride, 16-byte aligned) gets the bits[i] bits from bit off[i] of src, in 16-byte units; the bits behind them in
// the last unit are zero (rows carry KZ_STREAM_SLACK bytes behind their streams).  Nothing outside src[0 .. n) is read: units
// near either end of src load bytewise.
// the unit u (16 bytes) of a row: the bits from bit o + 128 u of src[0 .. n), zero behind the row's W bits
__device__ __forceinline__ uint4 knz_unpack_unit(const u8* __restrict__ src, int64_t n, int64_t o, int64_t W, int64_t u) {
  const int64_t sb = o + (u << 7);
  const int sh = (int)(sb & 7);
  const u8* p = src + (sb >> 3);
  const u8* al = (const u8*)((uintptr_t)p & ~(uintptr_t)3);
  uint4 v;
  if (al >= src && al + knz_window(p, sh) <= src + n) v = knz_load128(p, sh);
  else {
    u32 o4[4];
    const int64_t by = sb >> 3;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      u32 x = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int64_t c = by + q * 4 + t;
        const u32 b0 = c < n ? src[c] : 0u, b1 = (sh && c + 1 < n) ? src[c + 1] : 0u;
        x |= (((b0 << sh) | (b1 >> (8 - sh))) & 0xFFu) << (8 * t);
      }
      o4[q] = x;
    }
    v = make_uint4(o4[0], o4[1], o4[2], o4[3]);
  }
  const int64_t left = W - (u << 7);                                                 // bits of this unit that belong to the block
  if (left < 128) {
    u32* c = (u32*)&v;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t l = left - 32 * q;
      const u32 keepBE = l >= 32 ? ~0u : (l <= 0 ? 0u : ~0u << (32 - (int)l));       // mask on the big-endian view
      c[q] &= __builtin_bswap32(keepBE);
    }
  }
  return v;
}
__global__ void __launch_bounds__(256) k_knz_unpack(const u8* __restrict__ src, int64_t n, const int64_t* __restrict__ off, const int64_t* __restrict__ bits, int nb,
                                                    u8* __restrict__ rows, int64_t stride) {
  for (int i = blockIdx.y; i < nb; i += gridDim.y) {
    const int64_t W = bits[i], o = off[i];
    const int64_t units = (((W + 7) >> 3) + 15) >> 4;
    u8* row = rows + (int64_t)i * stride;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x)
      *(uint4*)(row + (u << 4)) = knz_unpack_unit(src, n, o, W, u);
  }
}

// ==== many streams in one call (kz_compress_many_device / kz_decompress_many_device) =========================================
// The same four steps with a table entry per segment, slot or row that carries its own bounds: a launch serves every stream of a
// group, and nothing is read outside a stream's own segment or written outside its own slot, wherever the other streams lie.

// ---- the unit of every byte copy here (k_knz_gather / k_knz_scatter, k_knz_read, k_knz_write) ---------------------------------------
// One 16-byte aligned unit of the destination side of a copy of len bytes from s to d, any alignment on both sides: ub = the unit's
// first byte as an index into the range (may be < 0, and ub + 16 may be > len: the unit's bytes outside the range are not touched).
// A whole unit is one wide store of aligned 32-bit loads if that load window stays inside [wlo, whi), the memory around s that may
// be read; any other unit goes bytewise, the range's own bytes only.
__device__ __forceinline__ void knz_copy_unit(u8* __restrict__ d, const u8* __restrict__ s, int64_t len, int64_t ub, const u8* wlo, const u8* whi) {
  const int64_t lo = ub < 0 ? 0 : ub, hi = ub + 16 > len ? len : ub + 16;
  if (lo >= hi) return;
  if (hi - lo == 16) {
    const u8* p = s + lo;
    const u8* al = (const u8*)((uintptr_t)p & ~(uintptr_t)3);
    if (al >= wlo && al + knz_window(p, 0) <= whi) { *(uint4*)(d + lo) = knz_load128(p, 0); return; }
  }
  for (int64_t b = lo; b < hi; b++) d[b] = s[b];
}

// ---- ragged copy: gather (segments -> encoder rows) and scatter (decoded rows -> slots) -----------------------------------------
// Entry r: t[r].len bytes from from[t[r].src ..] to to[t[r].dst ..], any alignment on both sides.  Output-centric like the pack: a
// lane owns one 16-byte aligned unit of the destination range (knz_copy_unit); the loads stay inside [src, src + len).
__device__ __forceinline__ void knz_ragged(const u8* __restrict__ from, const KnzCopy* __restrict__ t, int nr, u8* __restrict__ to) {
  for (int r = blockIdx.y; r < nr; r += gridDim.y) {
    const int64_t len = t[r].len;
    if (len <= 0) continue;
    const u8* s = from + t[r].src;
    u8* d = to + t[r].dst;
    const uintptr_t A0 = (uintptr_t)d & ~(uintptr_t)15;
    const int64_t units = (int64_t)(((uintptr_t)(d + len) - A0 + 15) >> 4);
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x)
      knz_copy_unit(d, s, len, (int64_t)(A0 - (uintptr_t)d) + (u << 4), s, s + len);
  }
}
__global__ void __launch_bounds__(256) k_knz_gather(const u8* __restrict__ src, const KnzCopy* __restrict__ t, int nr, u8* __restrict__ rows) { knz_ragged(src, t, nr, rows); }
__global__ void __launch_bounds__(256) k_knz_scatter(const u8* __restrict__ rows, const KnzCopy* __restrict__ t, int nr, u8* __restrict__ dst) { knz_ragged(rows, t, nr, dst); }

// ---- read: segments of decoded rows -> their places in dst (kz_read_bytes_device) -------------------------------------------------
// Segment j (kz_knz_host.h: KnzReadSeg) is seg[j].len bytes from byte seg[j].off of the row rows + seg[j].slot * stride (rowLen bytes
// of it are the block's) to dst + seg[j].dst, any alignment on both sides; from a few bytes to a whole block each, up to a million
// of them.  No workgroup per segment: the launch's work is the 16-byte aligned destination units of all its segments, one segment
// after the other (seg[j].unit0 = the first of segment j, a prefix sum that grows strictly with j; the launch owns units
// [unitBase, unitBase + units), seg[0].unit0 == unitBase).  A lane takes a unit, finds its segment by binary search on unit0 and copies
// the unit (knz_copy_unit) with the row as the window of its aligned loads.  A unit of memory that two segments share is visited once per
// segment, so every byte has one writer and no lane writes a byte that is not its segment's.  A segment whose len was cut after
// unit0 was summed (knz_read_settle) has units with nothing in them: they are skipped.
// The 64 units of a wave lie side by side and in one segment or a few neighbours: the wave searches once for its first and once for
// its last unit with wave-uniform arguments, a lane then only between the two (k_knz_splice's scheme).
template <class T> __device__ __forceinline__ int knz_read_find(const T* __restrict__ seg, int lo, int hi, int64_t u) {   // the last j in lo .. hi with unit0 <= u (seg[lo]'s is)
  int a = lo + 1, b = hi + 1;
  while (a < b) { const int m = (a + b) >> 1; if (seg[m].unit0 <= u) a = m + 1; else b = m; }
  return a - 1;
}
// the segment of unit u among seg[0 .. ns), by that scheme: the table's address stays the kernel's argument in all three searches
template <class T> __device__ __forceinline__ int knz_wave_find(const T* __restrict__ seg, int ns, int64_t u) {
  const int64_t u0 = knz_first_lane(u);                                               // the wave's units: at most 64 in a row from its first lane's
  const int jlo = knz_read_find(seg, 0, ns - 1, u0);
  int jhi = jlo;                                                                      // (every segment has a unit: 63 units on are at most 63 segments on)
  if (jlo + 1 < ns && seg[jlo + 1].unit0 <= u0 + 63) jhi = knz_read_find(seg, jlo + 1, jlo + 63 < ns - 1 ? jlo + 63 : ns - 1, u0 + 63);
  return knz_read_find(seg, jlo, jhi, u);
}
__global__ void __launch_bounds__(256) k_knz_read(const u8* __restrict__ rows, int64_t stride, int rowLen, const KnzReadSeg* __restrict__ seg, int ns,
                                                  u8* __restrict__ dst, int64_t unitBase, int64_t units) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < units; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = unitBase + v;
    const KnzReadSeg g = seg[knz_wave_find(seg, ns, u)];
    u8* d = dst + g.dst;
    const uintptr_t A0 = (uintptr_t)d & ~(uintptr_t)15;
    const int64_t ub = (int64_t)(A0 - (uintptr_t)d) + ((u - g.unit0) << 4);
    if (ub >= g.len) continue;                                                        // a unit of a segment that was cut: before the row's address is formed
    const u8* row = rows + (int64_t)g.slot * stride;
    knz_copy_unit(d, row + g.off, g.len, ub, row, row + rowLen);
  }
}

// ---- write: segments of the caller's new bytes -> their places in decoded rows (kz_write_bytes_device) ------------------------------
// k_knz_read's mirror image.  Segment j (kz_knz_host.h: KnzWriteSeg) is seg[j].len bytes from data + seg[j].src (any alignment) to
// byte seg[j].off of the row rows + seg[j].slot * stride (rows 16-byte aligned, stride a multiple of 16).  The launch's work is the
// 16-byte aligned units of the ROW side of all its segments, one segment after the other (seg[j].unit0, the launch owns
// [unitBase, unitBase + units), seg[0].unit0 == unitBase); a lane finds its segment with the read's wave-narrowed search
// (knz_wave_find) and copies the unit (knz_copy_unit) with data[0 .. dataLen) as the window of its aligned loads.  The plan made the segments disjoint (the later range has already won there), so
// every byte of a row has one writer and no order between lanes, launches or segments is needed; bytes of a row that no segment
// covers keep what the decode left in them.
__global__ void __launch_bounds__(256) k_knz_write(const u8* __restrict__ data, int64_t dataLen, const KnzWriteSeg* __restrict__ seg, int ns,
                                                   u8* __restrict__ rows, int64_t stride, int64_t unitBase, int64_t units) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < units; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = unitBase + v;
    const KnzWriteSeg g = seg[knz_wave_find(seg, ns, u)];
    u8* d = rows + (int64_t)g.slot * stride + g.off;
    const uintptr_t A0 = (uintptr_t)d & ~(uintptr_t)15;
    knz_copy_unit(d, data + g.src, g.len, (int64_t)(A0 - (uintptr_t)d) + ((u - g.unit0) << 4), data, data + dataLen);
  }
}

// ---- pack: the blocks of many streams -> their slots -----------------------------------------------------------------------------
// k_knz_pack's scheme over the slots of a group.  Stream s owns bytes [0, (endBit + 7) / 8) of its slot dst + seg[s].dst: the stream
// header (seg[s].hdr, a whole number of bytes), the fields of blk[blk0 .. blk0 + nblk) (pay counted from the slot's first bit), zeros
// up to endBit (the end marker) and to the end of the last byte.  The launch's units are the slots' 16-byte aligned units one slot
// after the other (seg[s].unit0 = the first of slot s, growing with s, seg[0].unit0 = 0): a lane finds its slot by binary search.
// Two slots may share an aligned unit of memory: each has a unit of its own for it and writes its own bytes only.  Every stream
// starts on a byte, so no byte is read back.
__global__ void __launch_bounds__(256) k_knz_pack_many(const u8* __restrict__ rows, const KnzSeg* __restrict__ seg, int ns, const KnzBlk* __restrict__ blkAll,
                                                       u8* dst, int64_t units) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    int s = 0;
    {
      int a = 0, b = ns;                                                            // invariant: unit0 of slots < a is <= u
      while (a < b) { const int m = (a + b) >> 1; if (seg[m].unit0 <= u) a = m + 1; else b = m; }
      s = a > 0 ? a - 1 : 0;
    }
    u8* d = dst + seg[s].dst;
    const int64_t lastByte = (seg[s].endBit + 7) >> 3;
    const int hdrBytes = seg[s].hdrBytes;
    const KnzBlk* blk = blkAll + seg[s].blk0;
    const int nb = seg[s].nblk;
    const uintptr_t A0 = (uintptr_t)d & ~(uintptr_t)15;
    const int64_t ub = (int64_t)(A0 - (uintptr_t)d) + ((u - seg[s].unit0) << 4);     // the unit's first byte as an index into the slot (may be < 0)
    const int64_t lo = ub < 0 ? 0 : ub, hi = ub + 16 > lastByte ? lastByte : ub + 16;
    if (lo >= hi) continue;
    const int64_t pos0 = lo << 3;
    int j = knz_find_field(blk, nb, pos0);
    if (hi - lo == 16 && knz_wide_unit(rows, blk, nb, j, pos0, hi << 3, d + lo)) continue;
    for (int64_t b = lo; b < hi; b++) {
      if (b < hdrBytes) { d[b] = seg[s].hdr[b]; continue; }
      d[b] = knz_compose_byte(rows, blk, nb, j, b << 3, (b + 1) << 3, 0u);
    }
  }
}

// ---- splice: blocks of existing streams and recoded rows -> bit ranges in many slots (kz_write_bytes_many_device) --------------------
// k_knz_splice's copy with many destinations in one launch.  Span s (kz_internal.h: KnzSpan) owns the bits [startBit, endBit) of the
// slot dst + sp[s].dst: the stream header when it is the stream's first span (sp[s].hdr, a whole number of bytes; startBit == 0), the
// fields of its pieces pcAll[piece0 .. piece0 + npieces) back to back (pay counted from the slot's first bit; a kept block lies in its
// own stream inside src, a recoded one in an encoder row named by its distance from src), zeros up to endBit and to the end of the
// last byte.  A span may have no piece: the header alone, or the end marker alone.  No staging rows for kept blocks: a payload bit is
// loaded once and stored once.
// The launch's work is the 16-byte aligned units of all its spans, one span after the other (sp[s].unit0, a prefix sum that grows
// strictly with s, sp[0].unit0 == 0).  A lane takes a unit and finds its span with the read's wave-narrowed search; the piece inside
// the span likewise when the whole wave is inside one span (k_knz_splice's scheme: its arguments are wave-uniform then), else by a
// search of its own.  A unit wholly inside one payload is one wide store of aligned loads that stay inside the piece's own source
// bounds; everything else is composed bytewise.
// Two spans of a launch never share a byte (every stream has one span per launch at the most, and slots do not overlap), but
// neighbouring slots may share an aligned unit of memory: each span has a unit of its own for it and writes its own bytes only.  A
// span that starts in mid-byte keeps that byte's high bits: they are the same stream's previous span, written by an earlier launch on
// the same HIP stream with the spare bits zero; only the lane of the span's first unit reads and writes that byte.
__global__ void __launch_bounds__(256) k_knz_splice_many(const u8* __restrict__ src, const KnzSpan* __restrict__ sp, int ns, const KnzPiece* __restrict__ pcAll,
                                                         u8* dst, int64_t units) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u0 = knz_first_lane(u);                                             // the wave's units: at most 64 in a row from its first lane's
    const int slo = knz_read_find(sp, 0, ns - 1, u0);
    int shi = slo;                                                                    // (every span has a unit: 63 units on are at most 63 spans on)
    if (slo + 1 < ns && sp[slo + 1].unit0 <= u0 + 63) shi = knz_read_find(sp, slo + 1, slo + 63 < ns - 1 ? slo + 63 : ns - 1, u0 + 63);
    const int s = knz_read_find(sp, slo, shi, u);
    const int64_t startBit = sp[s].startBit, endBit = sp[s].endBit;
    const int hdrBytes = sp[s].hdrBytes;
    const KnzPiece* pc = pcAll + sp[s].piece0;
    const int np = sp[s].npieces;
    u8* d = dst + sp[s].dst;
    const int64_t firstByte = startBit >> 3, lastByte = (endBit + 7) >> 3;           // [firstByte, lastByte) of the slot is written
    const uintptr_t A0 = (uintptr_t)(d + firstByte) & ~(uintptr_t)15;
    const int64_t ub = (int64_t)(A0 - (uintptr_t)d) + ((u - sp[s].unit0) << 4);       // the unit's first byte as an index into the slot (may be < firstByte)
    const int64_t lo = ub < firstByte ? firstByte : ub, hi = ub + 16 > lastByte ? lastByte : ub + 16;
    if (lo >= hi) continue;
    const int64_t pos0 = (lo == firstByte) ? startBit : (lo << 3);
    int j;
    if (slo == shi) {                                                                 // the wave's 64 units lie side by side in one span
      const int64_t ub0 = knz_first_lane(ub);
      const int jlo = knz_find_field(pc, np, ub0 < firstByte ? startBit : (ub0 << 3));
      const int jhi = knz_find_field(pc, np, (ub0 + 63 * 16) << 3);
      j = knz_find_between(pc, jlo, jhi, pos0);
    } else j = knz_find_field(pc, np, pos0);
    if (hi - lo == 16 && knz_wide_unit(src, pc, np, j, pos0, hi << 3, d + lo)) continue;
    int64_t pos = pos0;
    for (int64_t b = lo; b < hi; b++) {
      const int64_t bend = (b + 1) << 3;
      if (b < hdrBytes) { d[b] = sp[s].hdr[b]; pos = bend; continue; }
      const u32 acc = (pos & 7) ? d[b] & (0xFFu << (8 - (int)(pos & 7))) : 0u;        // only the span's first byte
      d[b] = knz_compose_byte(src, pc, np, j, pos, bend, acc);
      pos = bend;
    }
  }
}

// ---- heads: the first bytes of every stream, for the host's header parse -----------------------------------------------------------
// heads[32 s + i] = byte i of stream s for i < min(26, n) (the longest stream header), zero behind that
__global__ void __launch_bounds__(256) k_knz_heads(const u8* __restrict__ src, const KnzSrc* __restrict__ t, int ns, u8* __restrict__ heads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)ns * 32) return;
  const int s = (int)(i >> 5), k = (int)(i & 31);
  heads[i] = (k < 26 && k < t[s].n) ? src[t[s].off + k] : (u8)0;
}

// ---- walk: one lane per stream -----------------------------------------------------------------------------------------------------
// k_knz_walk's loop and stop reasons for stream s = src[t[s].off .. + t[s].n) from bit t[s].startBit, at most t[s].maxCount blocks;
// res[3 s ..] = (blocks recorded whole, bit position, reason).  Entry i of the stream goes to index t[s].base + i of off / bits / hdr
// when i < t[s].cap: the count pass runs with cap = 0 and writes res only, the fill pass with the counts' exclusive scan as base.
// Bit offsets count from the stream's own first bit.
__global__ void __launch_bounds__(64) k_knz_walk_many(const u8* __restrict__ src, const KnzSrc* __restrict__ t, int ns,
                                                      int64_t* __restrict__ off, int64_t* __restrict__ bits, u64* __restrict__ hdr, int64_t* __restrict__ res) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  knz_walk_stream(src + t[s].off, t[s].n, t[s].startBit, t[s].maxCount, t[s].cap, t[s].base, off, bits, hdr, res + 3 * s);
}

// ---- unpack: the blocks of many streams -> byte-aligned rows ---------------------------------------------------------------------
// k_knz_unpack with the bounds of each row's own stream: row r (rows + t[r].row, 16-byte aligned) gets t[r].bits bits from bit
// t[r].off of src[t[r].seg .. + t[r].n), and nothing outside that stream is read, not even bytes of a neighbour in the same buffer
__global__ void __launch_bounds__(256) k_knz_unpack_many(const u8* __restrict__ srcAll, const KnzRow* __restrict__ t, int nr, u8* __restrict__ rows) {
  for (int i = blockIdx.y; i < nr; i += gridDim.y) {
    const u8* src = srcAll + t[i].seg;
    const int64_t n = t[i].n, W = t[i].bits, o = t[i].off;
    const int64_t units = (((W + 7) >> 3) + 15) >> 4;
    u8* row = rows + t[i].row;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x)
      *(uint4*)(row + (u << 4)) = knz_unpack_unit(src, n, o, W, u);
  }
}

// ==== scan: the blocks of a stream found without the walk (kz_knz_scan_device) ================================================
// The rule (accept, final: kz_knz_host.h, one definition for host and device) asked at every bit position behind the stream header,
// then the link step over the accepted positions, which are sparse (1.5 to 7 in 10^4 positions of random bytes, by the stream's block size).

// ---- pass 1: every bit position --------------------------------------------------------------------------------------------------
// A workgroup takes a tile of KNZ_SCAN_TILE bytes of MEMORY (tiles start at multiples of the tile size from the 16-byte aligned
// address at or below src, so that the loads are aligned words whatever src's alignment is; what a tile holds in front of src or behind
// src + n reads as zero and is no position) and the 16 bytes behind it (the test looks at no more than 16 bytes from q's byte on), as
// big-endian words in LDS.  Lanes take consecutive bytes, eight positions each, 16 bytes a lane per tile.  The count form leaves the
// tile's accepted positions in cnt[t]; the write form, behind the exclusive scan tileOff of those counts, stores them in ascending q
// from index tileOff[t] on: positions ascend with (byte, bit), that is with (round, lane, bit), so a round's lanes take their places by
// a prefix sum over the workgroup.  Nothing outside src[0 .. n) is read: a word is loaded whole only if it lies inside, else bytewise.
#define KNZ_SCAN_TILE 4096
#define KNZ_SCAN_WORDS (KNZ_SCAN_TILE / 4 + 4)
// the exclusive prefix sum of c over the workgroup's 256 lanes and its total (ws: 4 ints of LDS; every lane calls, two barriers)
__device__ __forceinline__ int knz_block_excl(int c, int* ws, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
  if (lane == 63) ws[wv] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) { const int s = ws[w]; if (w < wv) base += s; total += s; }
  __syncthreads();
  return base + incl - c;
}
template <bool WRITE>
__device__ __forceinline__ void knz_scan_tiles(const u8* __restrict__ src, int64_t n, const KnzScanRule& R, int64_t nTiles, int32_t* __restrict__ cnt,
                                               const int64_t* __restrict__ tileOff, int64_t* __restrict__ oq, int64_t* __restrict__ opay, int64_t* __restrict__ oW) {
  __shared__ u32 win[KNZ_SCAN_WORDS];
  __shared__ int ws[4];
  const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)n, A0 = lo & ~(uintptr_t)15;
  for (int64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
    const uintptr_t ta = A0 + (uintptr_t)t * KNZ_SCAN_TILE;
    for (int w = threadIdx.x; w < KNZ_SCAN_WORDS; w += 256) {
      const uintptr_t a = ta + 4 * (uintptr_t)w;
      u32 v = 0;
      if (a >= lo && a + 4 <= hi) v = __builtin_bswap32(*(const u32*)a);
      else {
#pragma unroll
        for (int k = 0; k < 4; k++) v = (v << 8) | ((a + k >= lo && a + k < hi) ? (u32) * (const u8*)(a + k) : 0u);
      }
      win[w] = v;
    }
    __syncthreads();
    int mine = 0;
    int64_t run = WRITE ? tileOff[t] : 0;
    for (int it = 0; it < KNZ_SCAN_TILE / 256; it++) {
      const int B = it * 256 + (int)threadIdx.x;
      const int64_t by = (int64_t)(ta - lo) + B;                                      // the byte's index in the stream (< 0: in front of it)
      u32 mask = 0;
      uint64_t a = 0, b = 0;
      if (by >= 0 && by < n && by * 8 + 7 >= R.hdrEnd) {
        const int wi = B >> 2, s = (B & 3) << 3;
        u32 w[5], o[4];
#pragma unroll
        for (int i = 0; i < 5; i++) w[i] = win[wi + i];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = s ? ((w[i] << s) | (w[i + 1] >> (32 - s))) : w[i];
        a = ((u64)o[0] << 32) | o[1];
        b = ((u64)o[2] << 32) | o[3];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          int64_t pay, W;
          if (by * 8 + k >= R.hdrEnd && knz_scan_accept(a, b, by * 8 + k, R, pay, W)) mask |= 1u << k;
        }
      }
      if (!WRITE) { mine += __popc(mask); continue; }
      int total;
      int64_t at = run + knz_block_excl(__popc(mask), ws, total);
      run += total;
      for (; mask; mask &= mask - 1, at++) {
        const int64_t q = by * 8 + (__ffs((int)mask) - 1);
        int64_t pay = 0, W = 0;
        knz_scan_prefix(a, b, q, R.nbits, pay, W);
        oq[at] = q; opay[at] = pay; oW[at] = W;
      }
    }
    if (!WRITE) {
      int total;
      knz_block_excl(mine, ws, total);
      if (threadIdx.x == 0) cnt[t] = total;
    }
    __syncthreads();                                                                  // the window is the next tile's
  }
}
__global__ void __launch_bounds__(256) k_knz_scan_count(const u8* __restrict__ src, int64_t n, KnzScanRule R, int64_t nTiles, int32_t* __restrict__ cnt) {
  knz_scan_tiles<false>(src, n, R, nTiles, cnt, nullptr, nullptr, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) k_knz_scan_write(const u8* __restrict__ src, int64_t n, KnzScanRule R, int64_t nTiles, const int64_t* __restrict__ tileOff,
                                                        int64_t* __restrict__ oq, int64_t* __restrict__ opay, int64_t* __restrict__ oW) {
  knz_scan_tiles<true>(src, n, R, nTiles, nullptr, tileOff, oq, opay, oW);
}
// out[j] = in[0] + .. + in[j - 1] for j in 0 .. m: the tiles' counts to their first indices, the keep flags to ranks.  One workgroup
// goes through the array in rounds of 4096 entries, four neighbours a lane, and carries the sum from round to round.
__global__ void __launch_bounds__(1024) k_knz_scan_sum(const int32_t* __restrict__ in, int64_t m, int64_t* __restrict__ out) {
  __shared__ int ws[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < m; base += 4096) {
    const int64_t j0 = base + 4 * tid;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = j0 + k < m ? in[j0 + k] : 0; s += v[k]; }
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    if (lane == 63) ws[wv] = incl;
    __syncthreads();
    int64_t at = carry + incl - s;
    int total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const int x = ws[w]; if (w < wv) at += x; total += x; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) if (j0 + k < m) { out[j0 + k] = at; at += v[k]; }
    carry += total;
  }
  if (tid == 0) out[m] = carry;
}

// ---- the link passes: over the A accepted positions, ascending in q --------------------------------------------------------------
// What knz_scan_link (kz_knz_host.h) defines, a lane per position.  link: sidx[i] = the entry at succ(i) = pay[i] + W[i], by binary
// search behind i, or -1, and then fin[i] = final(succ(i)).  run: fwd[i] = the positions on the path from i on, counted up to mc; keep[i]
// = 1 if that path has mc of them or ends in front of a final marker.  mark: from every i along its path, at most mc - 1 links: entry
// j, d links on, lies on a path of d + fwd[j] positions that starts at i, and is kept when those are mc (every lane stores the same 1).
// A path of mc positions through j has such a start no more than mc - 1 links in front of j, so this is the rule.  The work of run and
// mark grows with mc.
struct KnzScanCols { int64_t *q, *pay, *W, *sidx, *rank; int32_t *fwd, *fin, *keep; };
__global__ void __launch_bounds__(256) k_knz_scan_link(const u8* __restrict__ src, int64_t n, KnzScanCols c, int64_t A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  const int64_t s = c.pay[i] + c.W[i];
  int64_t lo = i + 1, hi = A;                                                       // invariant: q of entries < lo is < s
  while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (c.q[m] < s) lo = m + 1; else hi = m; }
  const bool hit = lo < A && c.q[lo] == s;
  uint64_t a = 0, b = 0;
  if (!hit) knz_scan_window(src, n, s >> 3, a, b);
  c.sidx[i] = hit ? lo : -1;
  c.fin[i] = (!hit && knz_scan_final(a, b, s, n << 3)) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_knz_scan_run(KnzScanCols c, int64_t A, int mc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  int64_t j = i;
  int len = 1;
  while (len < mc && c.sidx[j] >= 0) { j = c.sidx[j]; len++; }
  c.fwd[i] = len;
  c.keep[i] = (len >= mc || (c.sidx[j] < 0 && c.fin[j])) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_knz_scan_mark(KnzScanCols c, int64_t A, int mc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  int64_t j = c.sidx[i];
  for (int d = 1; d < mc && j >= 0; d++, j = c.sidx[j])
    if (d + c.fwd[j] >= mc) c.keep[j] = 1;
}
// The kept entries in ascending order, behind the exclusive scan `rank` of keep: entry i goes to index rank[i] if that is below cap,
// with next = the rank of the entry at its succ (kept with it), or KNZ_SCAN_END / _BROKEN.  res[0] = the kept entries, res[1] = head:
// the entry at hdrEnd if it is kept (the first of all then), else END / BROKEN by final(hdrEnd).
__global__ void __launch_bounds__(256) k_knz_scan_emit(const u8* __restrict__ src, int64_t n, int64_t hdrEnd, KnzScanCols c, int64_t A, int64_t cap,
                                                       int64_t* __restrict__ oq, int64_t* __restrict__ opay, int64_t* __restrict__ oW, int64_t* __restrict__ onext,
                                                       int64_t* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    uint64_t a, b;
    knz_scan_window(src, n, hdrEnd >> 3, a, b);
    res[0] = A > 0 ? c.rank[A] : 0;
    res[1] = (A > 0 && c.q[0] == hdrEnd && c.keep[0]) ? 0 : (knz_scan_final(a, b, hdrEnd, n << 3) ? KNZ_SCAN_END : KNZ_SCAN_BROKEN);
  }
  if (i >= A || !c.keep[i]) return;
  const int64_t r = c.rank[i];
  if (r >= cap) return;
  const int64_t j = c.sidx[i];
  oq[r] = c.q[i]; opay[r] = c.pay[i]; oW[r] = c.W[i];
  onext[r] = j >= 0 ? c.rank[j] : (c.fin[i] ? KNZ_SCAN_END : KNZ_SCAN_BROKEN);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
// the scan's steps (kz_knz_scan_device): the tiles' counts and their scan into d_tileOff[0 .. nTiles]; the accepted positions; the
// link passes and the ranks; the kept entries.  The columns of A entries (rank: A + 1) lie one after the other from d_cols on.
int64_t kz_knz_scan_tiles_of(const uint8_t* d_src, int64_t n) {
  const uintptr_t lo = (uintptr_t)d_src, A0 = lo & ~(uintptr_t)15;
  return (int64_t)((lo + (uintptr_t)n - A0 + KNZ_SCAN_TILE - 1) / KNZ_SCAN_TILE);
}
size_t kz_knz_scan_cols_bytes(int64_t A) { return (size_t)(5 * A + 1) * 8 + 3 * kz_align((size_t)A * 4, 8); }
static inline KnzScanCols knz_scan_cols(uint8_t* d_cols, int64_t A) {
  KnzScanCols c;
  int64_t* p = (int64_t*)d_cols;
  c.q = p; c.pay = p + A; c.W = p + 2 * A; c.sidx = p + 3 * A; c.rank = p + 4 * A;
  const size_t w = kz_align((size_t)A * 4, 8);
  uint8_t* z = (uint8_t*)(p + 5 * A + 1);
  c.fwd = (int32_t*)z; c.fin = (int32_t*)(z + w); c.keep = (int32_t*)(z + 2 * w);
  return c;
}
static inline dim3 knz_scan_grid(int64_t nTiles) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(nTiles, 1 << 20))); }
int kz_knz_scan_count(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const KnzScanRule& R, int64_t nTiles, int32_t* d_cnt, int64_t* d_tileOff) {
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_COUNT, k_knz_scan_count, knz_scan_grid(nTiles), dim3(256), d_src, n, R, nTiles, d_cnt);
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_SUM, k_knz_scan_sum, dim3(1), dim3(1024), (const int32_t*)d_cnt, nTiles, d_tileOff);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_scan_links(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const KnzScanRule& R, int64_t nTiles, const int64_t* d_tileOff, uint8_t* d_cols, int64_t A, int mc) {
  if (A <= 0) return 0;
  const KnzScanCols c = knz_scan_cols(d_cols, A);
  const dim3 g((unsigned)((A + 255) / 256));
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_WRITE, k_knz_scan_write, knz_scan_grid(nTiles), dim3(256), d_src, n, R, nTiles, d_tileOff, c.q, c.pay, c.W);
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_LINK, k_knz_scan_link, g, dim3(256), d_src, n, c, A);
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_RUN, k_knz_scan_run, g, dim3(256), c, A, mc);
  if (mc > 1) KZ_LAUNCH(ctx, KID_KNZ_SCAN_MARK, k_knz_scan_mark, g, dim3(256), c, A, mc);
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_SUM, k_knz_scan_sum, dim3(1), dim3(1024), (const int32_t*)c.keep, A, c.rank);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_scan_emit(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const KnzScanRule& R, uint8_t* d_cols, int64_t A, int64_t cap, int64_t* d_out, int64_t M, int64_t* d_res) {
  const KnzScanCols c = knz_scan_cols(d_cols, A);
  KZ_LAUNCH(ctx, KID_KNZ_SCAN_EMIT, k_knz_scan_emit, dim3((unsigned)std::max<int64_t>(1, (A + 255) / 256)), dim3(256), d_src, n, R.hdrEnd, c, A, cap,
            d_out, d_out + M, d_out + 2 * M, d_out + 3 * M, d_res);
  KZ_HIP(hipGetLastError());
  return 0;
}

static inline dim3 knz_pack_grid(int64_t units) { return dim3((unsigned)std::min<int64_t>((units + 255) / 256, 1 << 20)); }
static inline dim3 knz_unpack_grid(int nb, int64_t maxBytes) {
  const int64_t units = (maxBytes + 15) >> 4;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 255) / 256, 1 << 16)), (unsigned)std::min(nb, KZ_MAX_BATCH));
}
int kz_knz_pack(kz_ctx* ctx, const uint8_t* d_rows, const KnzBlk* d_blk, int nb, uint8_t* d_dst, int64_t startBit, int64_t endBit) {
  if (endBit <= startBit) return 0;
  const int64_t units = (((endBit + 7) >> 3) - (startBit >> 3) + 15 + 15) >> 4;
  KZ_LAUNCH(ctx, KID_KNZ_PACK, k_knz_pack, knz_pack_grid(units), dim3(256), d_rows, d_blk, nb, d_dst, startBit, endBit);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_walk(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t startBit, int maxCount, int64_t* d_off, int64_t* d_bits, uint64_t* d_hdr, int64_t* d_res) {
  KZ_LAUNCH(ctx, KID_KNZ_WALK, k_knz_walk, dim3(1), dim3(64), d_src, n, startBit, maxCount, d_off, d_bits, (u64*)d_hdr, d_res);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_check(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t hdrEnd, const int64_t* d_off, const int64_t* d_bits, int nb, uint64_t* d_hdr, int64_t* d_bad) {
  if (nb <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_CHECK, k_knz_check, dim3((nb + 255) / 256), dim3(256), d_src, n, hdrEnd, d_off, d_bits, nb, (u64*)d_hdr, d_bad);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_unpack(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const int64_t* d_off, const int64_t* d_bits, int nb, int64_t maxBytes, uint8_t* d_rows, int64_t stride) {
  if (nb <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_UNPACK, k_knz_unpack, knz_unpack_grid(nb, maxBytes), dim3(256), d_src, n, d_off, d_bits, nb, d_rows, stride);
  KZ_HIP(hipGetLastError());
  return 0;
}

int kz_knz_check_many(kz_ctx* ctx, const uint8_t* d_src, const KnzPiece* d_pc, int np, int32_t* d_bad) {
  if (np <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_CHECK_MANY, k_knz_check_many, dim3((np + 255) / 256), dim3(256), d_src, d_pc, np, d_bad);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_check_rows(kz_ctx* ctx, const uint8_t* d_src, const KnzCheckRow* d_t, int nr, uint64_t* d_hdr, int64_t* d_bad) {
  if (nr <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_CHECK_ROWS, k_knz_check_rows, dim3((nr + 255) / 256), dim3(256), d_src, d_t, nr, (u64*)d_hdr, d_bad);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_splice_launch(kz_ctx* ctx, const uint8_t* d_src, const KnzPiece* d_pc, int np, uint8_t* d_dst, int64_t startBit, int64_t endBit) {
  if (endBit <= startBit) return 0;
  const int64_t units = (((endBit + 7) >> 3) - (startBit >> 3) + 15 + 15) >> 4;
  KZ_LAUNCH(ctx, KID_KNZ_SPLICE, k_knz_splice, knz_pack_grid(units), dim3(256), d_src, d_pc, np, d_dst, startBit, endBit);
  KZ_HIP(hipGetLastError());
  return 0;
}

static inline dim3 knz_ragged_grid(int nr, int64_t maxLen) {
  const int64_t units = ((maxLen + 15) >> 4) + 1;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 255) / 256, 1 << 16)), (unsigned)std::min(nr, KZ_MAX_BATCH));
}
int kz_knz_gather(kz_ctx* ctx, const uint8_t* d_src, const KnzCopy* d_t, int nr, int64_t maxLen, uint8_t* d_rows) {
  if (nr <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_GATHER, k_knz_gather, knz_ragged_grid(nr, maxLen), dim3(256), d_src, d_t, nr, d_rows);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_scatter(kz_ctx* ctx, const uint8_t* d_rows, const KnzCopy* d_t, int nr, int64_t maxLen, uint8_t* d_dst) {
  if (nr <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_SCATTER, k_knz_scatter, knz_ragged_grid(nr, maxLen), dim3(256), d_rows, d_t, nr, d_dst);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_pack_many(kz_ctx* ctx, const uint8_t* d_rows, const KnzSeg* d_seg, int ns, const KnzBlk* d_blk, uint8_t* d_dst, int64_t units) {
  if (ns <= 0 || units <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_PACK_MANY, k_knz_pack_many, knz_pack_grid(units), dim3(256), d_rows, d_seg, ns, d_blk, d_dst, units);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_splice_many(kz_ctx* ctx, const uint8_t* d_src, const KnzSpan* d_sp, int ns, const KnzPiece* d_pc, uint8_t* d_dst, int64_t units) {
  if (ns <= 0 || units <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_SPLICE_MANY, k_knz_splice_many, knz_pack_grid(units), dim3(256), d_src, d_sp, ns, d_pc, d_dst, units);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_heads(kz_ctx* ctx, const uint8_t* d_src, const KnzSrc* d_t, int ns, uint8_t* d_heads) {
  if (ns <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_HEADS, k_knz_heads, dim3((unsigned)(((int64_t)ns * 32 + 255) / 256)), dim3(256), d_src, d_t, ns, d_heads);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_walk_many(kz_ctx* ctx, const uint8_t* d_src, const KnzSrc* d_t, int ns, int64_t* d_off, int64_t* d_bits, uint64_t* d_hdr, int64_t* d_res) {
  if (ns <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_WALK_MANY, k_knz_walk_many, dim3((ns + 63) / 64), dim3(64), d_src, d_t, ns, d_off, d_bits, (u64*)d_hdr, d_res);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_unpack_many(kz_ctx* ctx, const uint8_t* d_src, const KnzRow* d_t, int nr, int64_t maxBytes, uint8_t* d_rows) {
  if (nr <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_UNPACK_MANY, k_knz_unpack_many, knz_unpack_grid(nr, maxBytes), dim3(256), d_src, d_t, nr, d_rows);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_read(kz_ctx* ctx, const uint8_t* d_rows, int64_t stride, int rowLen, const KnzReadSeg* d_seg, int ns, uint8_t* d_dst, int64_t unitBase, int64_t units) {
  if (ns <= 0 || units <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_READ, k_knz_read, knz_pack_grid(units), dim3(256), d_rows, stride, rowLen, d_seg, ns, d_dst, unitBase, units);
  KZ_HIP(hipGetLastError());
  return 0;
}
int kz_knz_write(kz_ctx* ctx, const uint8_t* d_data, int64_t dataLen, const KnzWriteSeg* d_seg, int ns, uint8_t* d_rows, int64_t stride, int64_t unitBase, int64_t units) {
  if (ns <= 0 || units <= 0) return 0;
  KZ_LAUNCH(ctx, KID_KNZ_WRITE, k_knz_write, knz_pack_grid(units), dim3(256), d_data, dataLen, d_seg, ns, d_rows, stride, unitBase, units);
  KZ_HIP(hipGetLastError());
  return 0;
}
