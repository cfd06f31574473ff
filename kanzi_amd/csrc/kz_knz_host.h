// kz_knz_host.h -- the host-only core of the .knz container: bit I/O, the stream header, the chain of block length prefixes, the
// block-header precheck and the check of an index entry, the scan's rule, link step and host loop, the plan of a splice and its host copy, the plan of a byte-addressed read,
// the merged plan of such a read over many streams, and the plan of a byte-addressed write, and the container's rules that every call must share, each written once.
// This is the part that parses untrusted input.  It needs no GPU and no HIP header, so that a plain C++ program can run it under
// the sanitizers (tools/knz_host_check.cpp, tools/knz_scan_check.cpp, tools/knz_read_check.cpp, tools/knz_write_check.cpp); kz_stream.hip and kz_stream_device.hip are its users.
// Layout: K/io/CompressedOutputStream.java (writeHeader :236-313, ordered block emission :1024-1035, end marker :483-493) and
// K/io/CompressedInputStream.java (readHeader :359-515, block length prefix :1127-1129).
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/kanzi_hip.h"

// what the host and the device share by one definition (the block-header precheck and the scan's rule): host code in a plain C++
// program, both in a HIP source
#ifdef __HIPCC__
#define KNZ_HD __host__ __device__
#else
#define KNZ_HD
#endif

struct HostBits {            // MSB-first writer (DefaultOutputBitStream.java:103-205)
  uint8_t* p; int64_t cap; uint64_t pos; bool overflow;
  void put(uint64_t v, int count) {
    if (count <= 0) return;
    if ((int64_t)((pos + count + 7) >> 3) > cap) { overflow = true; return; }
    if (count < 64) v &= ((1ULL << count) - 1);
    while (count > 0) {
      const int bitoff = (int)(pos & 7), room = 8 - bitoff;
      const int take = count < room ? count : room;
      const uint8_t bits = (uint8_t)((v >> (count - take)) & ((1u << take) - 1));
      if (bitoff == 0) p[pos >> 3] = 0;
      p[pos >> 3] |= (uint8_t)(bits << (room - take));
      pos += take; count -= take;
    }
  }
  void putBytes(const uint8_t* s, uint64_t nbits) {
    if (!nbits) return;
    if ((int64_t)((pos + nbits + 7) >> 3) > cap) { overflow = true; return; }
    const int sh = (int)(pos & 7);
    const uint64_t full = nbits >> 3;
    if (sh == 0) { if (full) memcpy(p + (pos >> 3), s, (size_t)full); pos += full << 3; }
    else {
      uint8_t* d = p + (pos >> 3);
      const int up = 8 - sh;
      if (full) {
        d[0] = (uint8_t)((d[0] & (0xFF << up)) | (s[0] >> sh));         // keep the bits already in the partial byte
        for (uint64_t i = 1; i < full; i++) d[i] = (uint8_t)((s[i - 1] << up) | (s[i] >> sh));   // no carried dependency: vectorises
        d[full] = (uint8_t)(s[full - 1] << up);
      }
      pos += full << 3;
    }
    const int r = (int)(nbits & 7);
    if (r) put((uint64_t)(s[full] >> (8 - r)), r);
  }
};
struct HostBitsIn {
  const uint8_t* p; uint64_t nbits; uint64_t pos; bool error;
  uint64_t get(int count) {
    if (count <= 0) return 0;
    if (pos + (uint64_t)count > nbits) { error = true; pos = nbits; return 0; }
    uint64_t v = 0;
    while (count > 0) {
      const int bitoff = (int)(pos & 7), room = 8 - bitoff;
      const int take = count < room ? count : room;
      v = (v << take) | (uint64_t)((p[pos >> 3] >> (room - take)) & ((1u << take) - 1));
      pos += take; count -= take;
    }
    return v;
  }
  void getBytes(uint8_t* d, uint64_t nb) {
    if (pos + nb > nbits) { error = true; pos = nbits; return; }
    const int sh = (int)(pos & 7);
    const uint64_t full = nb >> 3;
    const uint8_t* s = p + (pos >> 3);
    if (sh == 0) { if (full) memcpy(d, s, (size_t)full); }
    else for (uint64_t i = 0; i < full; i++) d[i] = (uint8_t)((s[i] << sh) | (s[i + 1] >> (8 - sh)));
    pos += full << 3;
    const int r = (int)(nb & 7);
    if (r) d[full] = (uint8_t)(get(r) << (8 - r));
  }
};
KNZ_HD inline uint32_t mix32(uint32_t c, uint32_t h, uint32_t v) { c ^= h * ~v; c = (c << 13) | (c >> 19); return c * 5u + 0x52DCE729u; }
static inline int ilog2(uint32_t x) { return 31 - __builtin_clz(x); }

// ---- the container's rules, one definition each ----
// width of the length field of a block of W bits (:1024-1035): the smallest lw >= 3 with W < 2^lw
static inline int knz_prefix_width(uint64_t W) { return W < 8 ? 3 : ilog2((uint32_t)(W >> 3)) + 4; }
// the 2-bit checksum field of the stream header <-> the ABI's checksumBits (0 / 32 / 64); -1: not a value of the ABI
static inline int knz_chk_kind(int32_t checksumBits) { return checksumBits == 0 ? 0 : (checksumBits == 32 ? 1 : (checksumBits == 64 ? 2 : -1)); }
static inline int32_t knz_chk_bits(int chkKind) { return chkKind == 1 ? 32 : (chkKind == 2 ? 64 : 0); }
// block sizes a writer takes (CompressedOutputStream.java:165-174)
static inline bool knz_block_size_ok(int32_t blockSize) { return blockSize >= 1024 && blockSize <= (1 << 30) && !(blockSize & 15); }
// Sequence length (TransformFactory.java:240-266): the non-zero 6-bit fields of the transform word, 1 at the least
static inline int knz_nb_functions(uint64_t transformType) {
  int nb = 0;
  for (int i = 0; i < 8; i++) if (((transformType >> (42 - 6 * i)) & 0x3F) != 0) nb++;
  return nb ? nb : 1;
}
// the decoder's staging row: a block's stream bound and 64 bytes of slack, in whole 256-byte lines
static inline int64_t knz_dec_row_stride(int32_t blockSize) {
  return (int64_t)(((size_t)blockSize + (size_t)(blockSize >> 3) + 1024 + 64 + 255) / 256 * 256);
}
// how many blocks may still start inside `room` bytes of destination
static inline int64_t knz_fit_blocks(int64_t room, int32_t blockSize) { return room <= 0 ? 0 : (room + blockSize - 1) / blockSize; }

// ---- stream header ----
static inline uint32_t header_cksum(int chkKind, int entropyType, uint64_t tt, int blockSize, int szMask, int64_t inputSize) {
  const uint32_t HASH = 0x1E35A7BDu;                          // CompressedOutputStream.java:293-309
  uint32_t c = HASH * (0x01030507u * 7u);
  c = mix32(c, HASH, (uint32_t)chkKind);
  c = mix32(c, HASH, (uint32_t)entropyType);
  c = mix32(c, HASH, (uint32_t)(tt >> 32));
  c = mix32(c, HASH, (uint32_t)tt);
  c = mix32(c, HASH, (uint32_t)blockSize);
  if (szMask > 0) { c = mix32(c, HASH, (uint32_t)((uint64_t)inputSize >> 32)); c = mix32(c, HASH, (uint32_t)inputSize); }
  return ((c >> 23) ^ (c >> 3)) & 0xFFFFFF;
}
static inline int write_stream_header(HostBits& bs, uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t n, int chkKind = 0) {
  bs.put(0x4B414E5A, 32); bs.put(7, 4); bs.put((uint64_t)chkKind, 2);
  bs.put(entropyType, 5); bs.put(transformType, 48); bs.put((uint32_t)blockSize >> 4, 28);
  int szMask = 0;
  if (n != 0 && n < (1LL << 48)) {
    if (n >= (1LL << 32)) szMask = 3;
    else { int64_t isz = n; if (isz > (1LL << 30)) { isz >>= 4; szMask++; } szMask += (ilog2((uint32_t)isz) >> 4) + 1; }
  }
  bs.put((uint64_t)szMask, 2);
  if (szMask > 0) bs.put((uint64_t)n, 16 * szMask);
  bs.put(0, 15);
  bs.put(header_cksum(chkKind, (int)entropyType, transformType, blockSize, szMask, n), 24);
  return szMask;
}
// Stream header, checked in the reference's order and with its codes (CompressedInputStream.java:359-478).
struct KnzHeader { int chkKind, entropyType, blockSize, szMask; uint64_t transformType; int64_t inputSize; };
static inline int read_stream_header(HostBitsIn& bs, KnzHeader& h, char* err, size_t errCap) {
  if (bs.get(32) != 0x4B414E5A) return -KZ_ERR_INVALID_FILE;                                    // :367-368
  const int bsVersion = (int)bs.get(4);
  if (bsVersion != 7) {                                                                            // :374-377; older layouts are not built here
    if (err) snprintf(err, errCap, "cannot read this version of the stream: %d (only 7 is built)", bsVersion);
    return -KZ_ERR_STREAM_VERSION;
  }
  h.chkKind = (int)bs.get(2);
  if (h.chkKind > 2) return -KZ_ERR_INVALID_FILE;                                               // :390-392
  h.entropyType = (int)bs.get(5);
  if (h.entropyType == 3 || h.entropyType > 9) return -KZ_ERR_INVALID_CODEC;                     // EntropyCodecFactory.getName :212-243
  h.transformType = bs.get(48);
  for (int i = 0; i < 8; i++) {                                                                  // TransformFactory.getName :368-449
    const int t = (int)((h.transformType >> (42 - 6 * i)) & 0x3F);
    if (t == 4 || t > 19) return -KZ_ERR_INVALID_CODEC;
  }
  h.blockSize = (int)(bs.get(28) << 4);
  if (h.blockSize < 1024 || h.blockSize > (1 << 30)) return -KZ_ERR_BLOCK_SIZE;                  // :419-422
  h.szMask = (int)bs.get(2);
  h.inputSize = h.szMask ? (int64_t)bs.get(16 * h.szMask) : 0;
  bs.get(15);
  const uint32_t ck = (uint32_t)bs.get(24);
  if (bs.error || ck != header_cksum(h.chkKind, h.entropyType, h.transformType, h.blockSize, h.szMask, h.inputSize))
    return -KZ_ERR_CRC_CHECK;                                                                    // :477-478
  return 0;
}
// the header's fields into the out-pointers of the index calls (each may be null)
static inline void knz_header_out(const KnzHeader& h, uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits) {
  if (transformType) *transformType = h.transformType;
  if (entropyType) *entropyType = (uint32_t)h.entropyType;
  if (blockSize) *blockSize = h.blockSize;
  if (inputSize) *inputSize = h.inputSize;
  if (checksumBits) *checksumBits = knz_chk_bits(h.chkKind);
}

// What a reading call derives from a parsed header, once (filled by knz_plan, kz_knz_stream.h): the transform count, the decoder's
// staging row, the decoder's batch NB and chunk CH, and the bit behind the stream header.
struct KnzPlan { KnzHeader h; int nbFunctions; int64_t iS; int64_t NB; int CH; int64_t hdrEnd; };

// ---- blocks ----
static inline void write_block(HostBits& bs, const uint8_t* stream, uint64_t written) {   // :1024-1035
  const int lw = knz_prefix_width(written);
  bs.put((uint64_t)(lw - 3), 5);
  bs.put(written, lw);
  bs.putBytes(stream, written);
}
static inline void write_end_marker(HostBits& bs) { bs.put(0, 5); bs.put(0, 3); }         // :491-492
// one length prefix (:1127-1129): 0 and W > 0 with bs at the block's payload, KNZ_PREFIX_END behind the end marker, or
// -KZ_ERR_READ_FILE when the prefix does not fit in the stream
enum { KNZ_PREFIX_END = 1 };
static inline int knz_read_prefix(HostBitsIn& bs, uint64_t& W) {
  const int lr = (int)bs.get(5) + 3;
  W = bs.get(lr);
  if (bs.error) return -KZ_ERR_READ_FILE;
  return W == 0 ? KNZ_PREFIX_END : 0;
}

// Restatement of DecodingTask.readBlockHeader + the two checks that follow it
// (CompressedInputStream.java:1025-1095, :1145-1164): the reference validates a block's header on the shared
// bit stream BEFORE it reads the payload, so a truncated or tampered stream is reported with the header's error
// (ERR_CRC_CHECK / ERR_BLOCK_SIZE / ERR_READ_FILE), not as a short read.  Returns 0 or -(error code).
// One definition for the host and the device: over hdr = the first 64 bits of the block's stream, left aligned (the header is 7
// bytes at the most; the device walk brings that word back), of which the stream holds the first `avail` (<= 64; what lies behind
// them in hdr is not looked at).
KNZ_HD inline int knz_precheck_word(uint64_t hdr, int avail, uint64_t W, int nbFunctions, int blockSize, int chkKind) {
  if (W < 8) return -KZ_ERR_BLOCK_SIZE;
  const uint32_t mode = avail >= 8 ? (uint32_t)(hdr >> 56) : 0u;      // (a mode byte that does not fit reads as 0, and fails below)
  uint32_t skipFlags = 0;
  bool hasSkip = false;
  if (mode & 0x80) {
    if (mode & 0x10) { if (nbFunctions > 4) hasSkip = true; else skipFlags = ((mode << 4) | 0x0F) & 0xFF; }
  } else if (mode & 0x10) hasSkip = true;
  else skipFlags = ((mode << 4) | 0x0F) & 0xFF;
  const int dataSize = 1 + (int)((mode >> 5) & 3);
  const int headerSize = 1 + (hasSkip ? 1 : 0) + dataSize + 1;
  if (W < (uint64_t)headerSize * 8) return -KZ_ERR_BLOCK_SIZE;
  if (avail < headerSize * 8) return -KZ_ERR_READ_FILE;
  int at = 8;
  if (hasSkip) { skipFlags = (uint32_t)(hdr >> 48) & 0xFF; at = 16; }
  const uint32_t preLen = (uint32_t)((hdr << at) >> (64 - 8 * dataSize));
  const uint32_t ck = (uint32_t)(hdr >> (56 - at - 8 * dataSize)) & 0xFF;
  const uint32_t HASH = 0x1E35A7BDu;
  uint32_t c = HASH * 0x01030507u;
  c = mix32(c, HASH, mode & 0xFF);
  c = mix32(c, HASH, skipFlags & 0xFF);
  c = mix32(c, HASH, preLen);
  c = mix32(c, HASH, (uint32_t)(W >> 32));
  c = mix32(c, HASH, (uint32_t)W);
  c = (c >> 23) ^ (c >> 3);
  if (ck != (c & 0xFF)) return -KZ_ERR_CRC_CHECK;
  int64_t maxTL = (int64_t)blockSize + blockSize / 2;
  if (maxTL < 2048) maxTL = 2048;
  if (maxTL > (1LL << 30)) maxTL = 1LL << 30;
  if ((int32_t)preLen < 0 || (int64_t)preLen > maxTL) return -KZ_ERR_READ_FILE;
  const int checksumSize = (chkKind == 2) ? 8 : (chkKind == 1 ? 4 : 0);
  if ((int64_t)((W + 7) >> 3) > (int64_t)preLen + headerSize + checksumSize) return -KZ_ERR_BLOCK_SIZE;
  return 0;
}
// the same for a reader that stands at the block's first bit
static inline int precheck_block_header(HostBitsIn bs /* by value: peek */, uint64_t W, int nbFunctions, int blockSize, int chkKind) {
  const int avail = bs.pos < bs.nbits ? (int)std::min<uint64_t>(64, bs.nbits - bs.pos) : 0;
  const uint64_t hdr = avail ? bs.get(avail) << (64 - avail) : 0;
  return knz_precheck_word(hdr, avail, W, nbFunctions, blockSize, chkKind);
}
// A reader's checks on one block of W bits whose payload starts at bit `at` of a stream of nbits bits, in the reader's order: the
// block header (peek: a reader at the payload's first bit), the staging-row bound, the payload's end inside the stream.  The indexed
// host read leaves the last one to knz_check_entry (checkEnd = false).  Returns 0 or -(error code).
static inline int knz_check_block(HostBitsIn peek, uint64_t W, uint64_t at, uint64_t nbits, const KnzPlan& P, bool checkEnd = true) {
  int rc = precheck_block_header(peek, W, P.nbFunctions, P.h.blockSize, P.h.chkKind);
  if (!rc && (int64_t)((W + 7) >> 3) > P.iS - 64) rc = -KZ_ERR_BLOCK_SIZE;
  if (!rc && checkEnd && at + W > nbits) rc = -KZ_ERR_READ_FILE;
  return rc;
}
// the next block of a serial reader: knz_read_prefix's results, then knz_check_block's code for the block; bs stays at the payload
static inline int knz_next_block(HostBitsIn& bs, const KnzPlan& P, uint64_t& W) {
  const int rc = knz_read_prefix(bs, W);
  return rc ? rc : knz_check_block(bs, W, bs.pos, bs.nbits, P);
}
// What becomes of a decoded block when `produced` bytes of a destination of dstCap bytes are taken: 0 (it is appended, :783-785) or
// the code that ends the stream, in the reader's order -- its status, "incorrectly decompressed" (:756-759), no room.
static inline int knz_block_verdict(const kz_block_result& r, int32_t blockSize, int64_t produced, int64_t dstCap) {
  if (r.status) return r.status;
  if (r.length > blockSize) return -KZ_ERR_PROCESS_BLOCK;
  if (produced + r.length > dstCap) return -KZ_ERR_WRITE_FILE;
  return 0;
}

// An index entry against the stream, on its own (no walk): the 5 + lr bits in front of bit `off` read (lr - 3, W) for some lr in
// 3 .. 34, and lie behind bit hdrEnd; W > 0 ends inside the stream
static inline bool knz_check_entry(const uint8_t* src, int64_t n, int64_t hdrEnd, int64_t off, int64_t W) {
  const int64_t nbits = n * 8;
  if (W <= 0 || W >= (1LL << 34) || off < hdrEnd + 8 || off > nbits || W > nbits - off) return false;
  const int lo = std::max(3, 64 - __builtin_clzll((unsigned long long)W));
  for (int lr = lo; lr <= 34; lr++) {
    const int64_t at = off - 5 - lr;
    if (at < hdrEnd) break;
    HostBitsIn t{src, (uint64_t)nbits, (uint64_t)at, false};
    if ((int)t.get(5) + 3 == lr && (int64_t)t.get(lr) == W) return true;
  }
  return false;
}

// ---- scan: the blocks of a stream found without the walk (kz_knz_scan / kz_knz_scan_device) ----
// The rule, asked at a bit position q of a stream of nbits bits whose header ends at bit hdrEnd: would a reader that stands at q
// accept a block?  accept(q): knz_read_prefix at q gives 0 and W > 0, and knz_check_block on the block behind it gives 0 (the header
// precheck, the staging-row bound, the payload's end inside the stream).  The test is local: 5 + lr <= 39 prefix bits and at most 56
// bits of block header, so with the (at most 7) bits in front of q in its byte it looks at no more than the 16 bytes from q's byte
// on.  a, b = those 16 bytes as two big-endian words, zeros where the stream has ended.
struct KnzScanRule { int64_t hdrEnd, nbits, maxBytes; int nbFunctions, blockSize, chkKind; };   // maxBytes: the staging-row bound, iS - 64
static inline KnzScanRule knz_scan_rule(const KnzHeader& h, int64_t hdrEnd, int64_t n) {
  return KnzScanRule{hdrEnd, n * 8, knz_dec_row_stride(h.blockSize) - 64, knz_nb_functions(h.transformType), h.blockSize, h.chkKind};
}
// the 64 bits from bit k (0 .. 127) of the 128-bit string a : b, zeros behind its end
KNZ_HD inline uint64_t knz_bits128(uint64_t a, uint64_t b, int k) {
  return k == 0 ? a : (k < 64 ? (a << k) | (b >> (64 - k)) : (k == 64 ? b : b << (k - 64)));
}
// the prefix at q: false when it does not fit; else pay = the bit behind it and W (0: the end marker's)
KNZ_HD inline bool knz_scan_prefix(uint64_t a, uint64_t b, int64_t q, int64_t nbits, int64_t& pay, int64_t& W) {
  if (q + 5 > nbits) return false;
  const uint64_t x = knz_bits128(a, b, (int)(q & 7));
  const int lr = (int)(x >> 59) + 3;
  pay = q + 5 + lr;
  if (pay > nbits) return false;
  W = (int64_t)((x << 5) >> (64 - lr));
  return true;
}
// accept(q), cheapest test first: the range of W, then the header's sizes and its checksum mix (knz_precheck_word)
KNZ_HD inline bool knz_scan_accept(uint64_t a, uint64_t b, int64_t q, const KnzScanRule& R, int64_t& pay, int64_t& W) {
  if (!knz_scan_prefix(a, b, q, R.nbits, pay, W)) return false;
  if (W < 8 || W > R.nbits - pay || ((W + 7) >> 3) > R.maxBytes) return false;
  const uint64_t hdr = knz_bits128(a, b, (int)(q & 7) + (int)(pay - q));
  return knz_precheck_word(hdr, W < 64 ? (int)W : 64, (uint64_t)W, R.nbFunctions, R.blockSize, R.chkKind) == 0;   // (W <= nbits - pay: that much of hdr is the stream's)
}
// final(s): the end marker at s, and the byte behind it is the stream's last (an end marker in the middle of the bytes is no end:
// runs of zeros are common inside payloads)
KNZ_HD inline bool knz_scan_final(uint64_t a, uint64_t b, int64_t s, int64_t nbits) {
  int64_t pay, W;
  return knz_scan_prefix(a, b, s, nbits, pay, W) && W == 0 && ((pay + 7) >> 3) == (nbits >> 3);
}
// a, b for the byte `by` of src[0 .. n)
KNZ_HD inline void knz_scan_window(const uint8_t* src, int64_t n, int64_t by, uint64_t& a, uint64_t& b) {
  a = b = 0;
  for (int i = 0; i < 8; i++) { a = (a << 8) | (by + i < n ? src[by + i] : 0u); b = (b << 8) | (by + 8 + i < n ? src[by + 8 + i] : 0u); }
}
enum { KNZ_SCAN_END = -1, KNZ_SCAN_BROKEN = -2 };                  // KZ_SCAN_END / KZ_SCAN_BROKEN (kanzi_hip.h)
static inline int knz_scan_args(const void* src, int64_t n, int32_t minChain, const int64_t* prefixBitOff, const int64_t* blockBitOff, const int64_t* blockBits,
                                const int64_t* next, int64_t cap, const int64_t* head) {
  if (!src || n < 0 || cap < 0 || minChain < 1 || !head || (cap > 0 && (!prefixBitOff || !blockBitOff || !blockBits || !next))) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
// Which accepted positions are kept (the link step, the definition that the device's link kernels restate).  q[], pay[], W[]: the A
// accepted positions in ascending q; succ(i) = pay[i] + W[i]; fin(s) = final(s).  A path is a run of accepted positions, each the
// succ of the one before; i is kept if it lies on a path of at least minChain positions, or if its path ends in front of a final
// marker.  sidx[i] = the entry at succ(i) or -1, fin[i] = final(succ(i)), keep[i] = 0 / 1.  (succ(i) > q[i]: one pass down gives
// what lies in front of i, one pass up what lies behind it.)
template <class F> static inline void knz_scan_link(const int64_t* q, const int64_t* pay, const int64_t* W, int64_t A, int64_t minChain, F fin_,
                                                    std::vector<int64_t>& sidx, std::vector<uint8_t>& fin, std::vector<uint8_t>& keep) {
  sidx.assign((size_t)A, -1); fin.assign((size_t)A, 0); keep.assign((size_t)A, 0);
  std::vector<int64_t> fwd((size_t)A, 1), back((size_t)A, 1);
  std::vector<uint8_t> reach((size_t)A, 0);
  for (int64_t i = A - 1; i >= 0; i--) {
    const int64_t s = pay[i] + W[i];
    const int64_t j = std::lower_bound(q + i + 1, q + A, s) - q;
    if (j < A && q[j] == s) { sidx[(size_t)i] = j; fwd[(size_t)i] = std::min<int64_t>(minChain, fwd[(size_t)j] + 1); reach[(size_t)i] = reach[(size_t)j]; }
    else reach[(size_t)i] = fin[(size_t)i] = fin_(s) ? 1 : 0;
  }
  for (int64_t i = 0; i < A; i++) {
    const int64_t j = sidx[(size_t)i];
    if (j >= 0) back[(size_t)j] = std::max(back[(size_t)j], std::min<int64_t>(minChain, back[(size_t)i] + 1));
    keep[(size_t)i] = (reach[(size_t)i] || back[(size_t)i] + fwd[(size_t)i] - 1 >= minChain) ? 1 : 0;   // (back[i] is final: every predecessor lies in front of i)
  }
}
// kz_knz_scan: every bit position behind the stream header, the link step, the kept entries in ascending order
static inline int64_t knz_scan_host(const uint8_t* src, int64_t n, int32_t minChain, uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize,
                                    int32_t* checksumBits, int64_t* prefixBitOff, int64_t* blockBitOff, int64_t* blockBits, int64_t* next, int64_t cap, int64_t* head) {
  { const int rc = knz_scan_args(src, n, minChain, prefixBitOff, blockBitOff, blockBits, next, cap, head); if (rc) return rc; }
  if (n < 20) return -KZ_ERR_INVALID_FILE;                         // (kz_knz_index's)
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, nullptr, 0); if (hrc) return hrc; }
  knz_header_out(h, transformType, entropyType, blockSize, inputSize, checksumBits);
  const KnzScanRule R = knz_scan_rule(h, (int64_t)bs.pos, n);
  std::vector<int64_t> q, pay, W;
  for (int64_t by = R.hdrEnd >> 3; by < n; by++) {
    uint64_t a, b;
    knz_scan_window(src, n, by, a, b);
    for (int k = 0; k < 8; k++) {
      int64_t p, w;
      if (by * 8 + k >= R.hdrEnd && knz_scan_accept(a, b, by * 8 + k, R, p, w)) { q.push_back(by * 8 + k); pay.push_back(p); W.push_back(w); }
    }
  }
  auto fin_ = [&](int64_t s) { uint64_t a, b; knz_scan_window(src, n, s >> 3, a, b); return knz_scan_final(a, b, s, R.nbits); };
  const int64_t A = (int64_t)q.size();
  std::vector<int64_t> sidx, rank((size_t)A + 1, 0);
  std::vector<uint8_t> fin, keep;
  knz_scan_link(q.data(), pay.data(), W.data(), A, minChain, fin_, sidx, fin, keep);
  for (int64_t i = 0; i < A; i++) rank[(size_t)i + 1] = rank[(size_t)i] + keep[(size_t)i];
  for (int64_t i = 0; i < A; i++) {
    const int64_t r = rank[(size_t)i];
    if (!keep[(size_t)i] || r >= cap) continue;
    prefixBitOff[r] = q[(size_t)i]; blockBitOff[r] = pay[(size_t)i]; blockBits[r] = W[(size_t)i];
    next[r] = sidx[(size_t)i] >= 0 ? rank[(size_t)sidx[(size_t)i]] : (fin[(size_t)i] ? KNZ_SCAN_END : KNZ_SCAN_BROKEN);   // (the entry at succ of a kept one is kept)
  }
  *head = (A > 0 && q[0] == R.hdrEnd && keep[0]) ? 0 : (fin_(R.hdrEnd) ? KNZ_SCAN_END : KNZ_SCAN_BROKEN);
  return rank[(size_t)A];
}

// ---- splice: a new stream out of blocks of existing streams (kz_knz_splice / kz_knz_splice_device) ----
// The plan of a splice, in the three steps both forms take in this order: the arguments, the sources' headers, and (behind the check
// of every piece against its own source: knz_check_entry on the host, k_knz_check_many on the device) the layout of the result.
// Only host arrays and the first bytes of every source are looked at, so the plan is the same code for both forms.
struct KnzSplice {
  KnzHeader h;                       // what the sources agree in (source 0's header)
  uint8_t hdr[32]; int64_t hdrBits;  // the result's stream header
  int64_t endBit;                    // the bit behind the end marker
};
static inline int knz_splice_args(const void* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nSrc, const int32_t* pieceSrc, const int64_t* pieceBitOff,
                                  const int64_t* pieceBits, int32_t nPieces, int64_t inputSize, const void* dst, int64_t dstCap) {
  if (!src || !srcOff || !srcLen || nSrc < 1 || nPieces < 0 || (nPieces > 0 && (!pieceSrc || !pieceBitOff || !pieceBits)) || inputSize < 0 || !dst || dstCap < 0)
    return -KZ_ERR_INVALID_PARAM;
  for (int s = 0; s < nSrc; s++) if (srcOff[s] < 0 || srcLen[s] < 0) return -KZ_ERR_INVALID_PARAM;
  for (int i = 0; i < nPieces; i++) if (pieceSrc[i] < 0 || pieceSrc[i] >= nSrc) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
// The header of every source (the first min(26, srcLen[s]) bytes of source s at heads + headOff[s]), each one parsed whether a piece
// names the source or not, and compared with source 0's; hdrEnd[s] = the bit behind it.  A header's fault is its code from
// read_stream_header; err (may be null) names the source.
static inline int knz_splice_sources(const uint8_t* heads, const int64_t* headOff, const int64_t* srcLen, int nSrc, KnzSplice& P, int64_t* hdrEnd, char* err, size_t errCap) {
  for (int s = 0; s < nSrc; s++) {
    HostBitsIn bs{heads + headOff[s], (uint64_t)std::min<int64_t>(srcLen[s], 26) * 8, 0, false};
    KnzHeader h;
    char why[96] = "";
    const int rc = read_stream_header(bs, h, why, sizeof(why));
    if (rc) { if (err) snprintf(err, errCap, "source %d: %s", s, why[0] ? why : "not a stream header"); return rc; }
    hdrEnd[s] = (int64_t)bs.pos;
    if (s == 0) { P.h = h; continue; }
    const char* what = h.transformType != P.h.transformType ? "the transform word" : (h.entropyType != P.h.entropyType ? "the entropy id" :
                       (h.blockSize != P.h.blockSize ? "the block size" : (h.chkKind != P.h.chkKind ? "the checksum kind" : nullptr)));
    if (what) { if (err) snprintf(err, errCap, "source %d differs from source 0 in %s", s, what); return -KZ_ERR_INVALID_PARAM; }
  }
  return 0;
}
static inline int knz_splice_mismatch(int64_t i, char* err, size_t errCap) {
  if (err) snprintf(err, errCap, "piece %lld does not match its source", (long long)i);
  return -KZ_ERR_INVALID_PARAM;
}
// The result of pieces that passed their checks (0 < W < 2^34): the stream header, pre[i] = the bit where piece i's prefix starts
// (pre[nPieces] = the end marker's), the end bit.  -KZ_ERR_WRITE_FILE when that is more than dstCap bytes: nothing has been written.
static inline int knz_splice_layout(const int64_t* pieceBits, int nPieces, int64_t inputSize, int64_t dstCap, KnzSplice& P, int64_t* pre) {
  HostBits hb{P.hdr, 32, 0, false};
  write_stream_header(hb, P.h.transformType, (uint32_t)P.h.entropyType, P.h.blockSize, inputSize, P.h.chkKind);
  P.hdrBits = (int64_t)hb.pos;
  int64_t pos = P.hdrBits;
  for (int i = 0; i < nPieces; i++) {
    pre[i] = pos;
    pos += 5 + knz_prefix_width((uint64_t)pieceBits[i]) + pieceBits[i];
    if (pos > (1LL << 62)) return -KZ_ERR_WRITE_FILE;
  }
  pre[nPieces] = pos;
  P.endBit = pos + 8;
  return ((P.endBit + 7) >> 3) > dstCap ? -KZ_ERR_WRITE_FILE : 0;
}
// kz_knz_splice_bound: the longest stream header, 5 + lw + W bits per piece, the end marker
static inline int64_t knz_splice_bound(const int64_t* pieceBits, int32_t nPieces) {
  if (nPieces < 0 || (nPieces > 0 && !pieceBits)) return -KZ_ERR_INVALID_PARAM;
  int64_t bits = 8;
  for (int i = 0; i < nPieces; i++) {
    if (pieceBits[i] < 0 || pieceBits[i] >= (1LL << 34)) return -KZ_ERR_INVALID_PARAM;
    bits += 5 + knz_prefix_width((uint64_t)pieceBits[i]) + pieceBits[i];
    if (bits > (1LL << 62)) return -KZ_ERR_INVALID_PARAM;
  }
  return 26 + ((bits + 7) >> 3);
}
// W bits from bit `off` of a stream of n bytes to the writer's position, whatever the two bit phases are.  The caller has checked
// that [off, off + W) lies inside the stream and that the writer has the room.
static inline void knz_copy_bits(HostBits& bs, const uint8_t* src, int64_t n, int64_t off, int64_t W) {
  uint8_t tmp[4096];
  HostBitsIn in{src, (uint64_t)n * 8, (uint64_t)off, false};
  while (W > 0) {
    const int64_t k = std::min<int64_t>(W, (int64_t)sizeof(tmp) * 8);
    in.getBytes(tmp, (uint64_t)k);
    bs.putBytes(tmp, (uint64_t)k);
    W -= k;
  }
}
// kz_knz_splice: the plan, with knz_check_entry on every piece, then per piece its minimal prefix and its payload bits copied from
// where they lie in their source.  Nothing is written before every check has passed.
static inline int64_t knz_splice_host(const uint8_t* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nSrc, const int32_t* pieceSrc,
                                      const int64_t* pieceBitOff, const int64_t* pieceBits, int32_t nPieces, int64_t inputSize, uint8_t* dst, int64_t dstCap) {
  { const int rc = knz_splice_args(src, srcOff, srcLen, nSrc, pieceSrc, pieceBitOff, pieceBits, nPieces, inputSize, dst, dstCap); if (rc) return rc; }
  KnzSplice P;
  std::vector<int64_t> hdrEnd((size_t)nSrc), pre((size_t)nPieces + 1);
  { const int rc = knz_splice_sources(src, srcOff, srcLen, nSrc, P, hdrEnd.data(), nullptr, 0); if (rc) return rc; }
  for (int i = 0; i < nPieces; i++) {
    const int s = pieceSrc[i];
    if (!knz_check_entry(src + srcOff[s], srcLen[s], hdrEnd[s], pieceBitOff[i], pieceBits[i])) return knz_splice_mismatch(i, nullptr, 0);
  }
  { const int rc = knz_splice_layout(pieceBits, nPieces, inputSize, dstCap, P, pre.data()); if (rc) return rc; }
  HostBits bs{dst, dstCap, 0, false};
  for (int64_t b = 0; b < (P.hdrBits >> 3); b++) bs.put(P.hdr[b], 8);
  for (int i = 0; i < nPieces; i++) {
    const int s = pieceSrc[i];
    const int lw = knz_prefix_width((uint64_t)pieceBits[i]);
    bs.put((uint64_t)(lw - 3), 5);
    bs.put((uint64_t)pieceBits[i], lw);
    knz_copy_bits(bs, src + srcOff[s], srcLen[s], pieceBitOff[i], pieceBits[i]);
  }
  write_end_marker(bs);
  return bs.overflow ? -KZ_ERR_WRITE_FILE : (int64_t)((bs.pos + 7) >> 3);
}

// ---- byte-addressed reads: many ranges of the original data in one call (kz_read_bytes / kz_read_bytes_device) ----
// The plan of such a call, from host arrays alone, so that both forms share it: block k of the index holds the original bytes
// [B[k], B[k + 1]), B = the caller's table or k * blockSize; range i owns dst[D[i], D[i] + rangeLen[i]), D = the running sum of the
// requested lengths.  A segment is one range cut with one block.  All sums are formed so that no int64 overflows: a range's end is
// never computed, its length is cut to what lies in front of the end of data instead.
struct KnzReadSeg {          // 32 bytes: the entry of k_knz_read's table
  int64_t dst;               // byte offset in dst
  int64_t unit0;             // the segment's first 16-byte aligned destination unit among the units of its chunk (prefix sum)
  int32_t slot;              // the block's row among the rows of its chunk
  int32_t off;               // byte offset in the block
  int32_t len;               // bytes (> 0 in the plan; knz_read_settle cuts it to what the block decoded to)
  int32_t range;             // the owning range
};
struct KnzReadPlan {
  int64_t end;                         // the end of data as the arguments give it: B[nIndex], or nIndex * blockSize without a table
  std::vector<int32_t> blocks;         // the distinct covering blocks, ascending; chunk c = blocks[c * CH .. (c + 1) * CH)
  std::vector<KnzReadSeg> segs;        // chunk by chunk; inside a chunk by dst, which is by range and then by block
  std::vector<int64_t> first;          // chunk c owns segs[first[c] .. first[c + 1])
  std::vector<int64_t> units;          // units[c] = the destination units of chunk c: what unit0 sums up to
};
// 16-byte aligned units of memory that len > 0 bytes from an address with (address mod 16) == phase touch
static inline int64_t knz_read_units(int64_t phase, int64_t len) { return (phase + len + 15) >> 4; }
static inline int knz_read_args(const void* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nIndex, const int64_t* rangeOff,
                                const int64_t* rangeLen, int32_t nRanges, const void* dst, int64_t dstCap, const int64_t* got) {
  if (!src || n < 0 || nIndex < 0 || nRanges < 0 || dstCap < 0 || (nIndex > 0 && (!blockBitOff || !blockBits))) return -KZ_ERR_INVALID_PARAM;
  if (nRanges > 0 && (!rangeOff || !rangeLen || !dst || !got)) return -KZ_ERR_INVALID_PARAM;
  for (int32_t i = 0; i < nRanges; i++) if (rangeOff[i] < 0 || rangeLen[i] < 0) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
// a caller's table of nIndex + 1 byte offsets: B[0] == 0 and 1 <= B[k + 1] - B[k] <= blockSize (B[k] >= 0 by induction, so the
// difference of an ascending pair cannot overflow)
static inline int knz_read_table(const int64_t* B, int32_t nIndex, int32_t blockSize) {
  if (!B) return 0;
  if (B[0] != 0) return -KZ_ERR_INVALID_PARAM;
  for (int32_t k = 0; k < nIndex; k++) if (B[k + 1] <= B[k] || B[k + 1] - B[k] > blockSize) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
// D[nRanges], or -KZ_ERR_WRITE_FILE when it is more than dstCap (a sum that leaves int64 is)
static inline int64_t knz_read_total(const int64_t* rangeLen, int32_t nRanges, int64_t dstCap) {
  int64_t D = 0;
  for (int32_t i = 0; i < nRanges; i++) {
    if (rangeLen[i] > dstCap - D) return -KZ_ERR_WRITE_FILE;
    D += rangeLen[i];
  }
  return D;
}
// The check of the length that block k decoded to, for both settles.  It must be B[k + 1] - B[k]; without a table blockSize, and any
// length up to blockSize for the last.  0, -KZ_ERR_PROCESS_BLOCK (more than a block) or -KZ_ERR_INVALID_FILE (another length).
static inline int knz_block_len_check(const int64_t* B, int32_t nIndex, int32_t blockSize, int32_t k, int64_t length) {
  const int64_t want = B ? B[k + 1] - B[k] : (k == nIndex - 1 ? -1 : blockSize);
  if (length > blockSize) return -KZ_ERR_PROCESS_BLOCK;
  return want >= 0 && length != want ? -KZ_ERR_INVALID_FILE : 0;
}
// the block that holds byte o of the data
static inline int64_t knz_block_of(const int64_t* B, int32_t nIndex, int32_t blockSize, int64_t o) {
  return B ? (std::upper_bound(B, B + nIndex + 1, o) - B) - 1 : o / blockSize;
}
// The bytes [at, at + left) of the data cut at block ends, k = the block that holds byte `at`: piece(k, off, len) per block, off = the
// piece's first byte in block k.
template <class F> static inline void knz_cut_at_blocks(const int64_t* B, int32_t blockSize, int64_t k, int64_t at, int64_t left, F piece) {
  for (; left > 0; k++) {
    const int64_t b0 = B ? B[k] : k * blockSize, b1 = B ? B[k + 1] : b0 + blockSize;
    const int64_t len = std::min<int64_t>(left, b1 - at);
    piece(k, at - b0, len);
    at += len; left -= len;
  }
}
// The segments of one range: bytes [o, o + len) of data that ends at `end`, cut at block ends, for the destination from byte d on.
// They go behind all (in dst order when the ranges come in dst order), the block of each behind blk.  A range of no bytes and one that
// starts at or behind `end` has no segment.
static inline void knz_read_cut(const int64_t* B, int32_t nIndex, int32_t blockSize, int64_t end, int64_t o, int64_t len, int64_t d, int32_t range,
                                std::vector<KnzReadSeg>& all, std::vector<int32_t>& blk) {
  const int64_t left = o < end ? std::min<int64_t>(len, end - o) : 0;
  if (left <= 0) return;
  knz_cut_at_blocks(B, blockSize, knz_block_of(B, nIndex, blockSize, o), o, left, [&](int64_t k, int64_t off, int64_t l) {
    all.push_back(KnzReadSeg{d, 0, 0, (int32_t)off, (int32_t)l, range});
    blk.push_back((int32_t)k);
    d += l;
  });
}
// The segments `all` (in dst order) split by chunk, stably: dst order stays inside every chunk.  place(i, c, slot): the chunk and the
// row in it of segment i's block.  Fills segs, first[0 .. nChunks] and units[0 .. nChunks) as KnzReadPlan holds them.
template <class F> static inline void knz_read_split(const std::vector<KnzReadSeg>& all, int64_t nChunks, int dstPhase, F place, std::vector<KnzReadSeg>& segs,
                                                     std::vector<int64_t>& first, std::vector<int64_t>& units) {
  first.assign((size_t)nChunks + 1, 0);
  units.assign((size_t)nChunks, 0);
  std::vector<int64_t> chunk(all.size());
  std::vector<int32_t> slot(all.size());
  for (size_t i = 0; i < all.size(); i++) {
    place(i, chunk[i], slot[i]);
    first[(size_t)chunk[i] + 1]++;
  }
  for (int64_t c = 0; c < nChunks; c++) first[(size_t)c + 1] += first[(size_t)c];
  std::vector<int64_t> fill(first.begin(), first.end() - 1);
  segs.resize(all.size());
  for (size_t i = 0; i < all.size(); i++) {
    const int64_t c = chunk[i];
    KnzReadSeg s = all[i];
    s.slot = slot[i];
    s.unit0 = units[(size_t)c];
    units[(size_t)c] += knz_read_units((dstPhase + s.dst) & 15, s.len);
    segs[(size_t)fill[(size_t)c]++] = s;
  }
}
// The plan.  The arguments have passed knz_read_args and knz_read_table; CH >= 1 = blocks per chunk; dstPhase = dst's address mod
// 16 (the host form passes 0: unit0 is the kernel's).  Ranges of no bytes and ranges that start at or behind P.end have no segment.
static inline void knz_read_plan(const int64_t* B, int32_t nIndex, int32_t blockSize, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                                 int CH, int dstPhase, KnzReadPlan& P) {
  P.end = B ? B[nIndex] : (int64_t)nIndex * blockSize;
  P.blocks.clear(); P.segs.clear(); P.first.assign(1, 0); P.units.clear();
  std::vector<KnzReadSeg> all;                                     // in range order: by dst
  std::vector<int32_t> blk;                                        // the block of all[i]
  int64_t D = 0;
  for (int32_t i = 0; i < nRanges; i++) {
    knz_read_cut(B, nIndex, blockSize, P.end, rangeOff[i], rangeLen[i], D, i, all, blk);
    D += rangeLen[i];                                              // (<= dstCap: knz_read_total)
  }
  P.blocks = blk;
  std::sort(P.blocks.begin(), P.blocks.end());
  P.blocks.erase(std::unique(P.blocks.begin(), P.blocks.end()), P.blocks.end());
  const int64_t nChunks = ((int64_t)P.blocks.size() + CH - 1) / CH;
  knz_read_split(all, nChunks, dstPhase, [&](size_t i, int64_t& c, int32_t& slot) {
    const int32_t rank = (int32_t)(std::lower_bound(P.blocks.begin(), P.blocks.end(), blk[i]) - P.blocks.begin());   // the block's place among the distinct blocks
    c = rank / CH; slot = rank % CH;
  }, P.segs, P.first, P.units);
}
// After cnt rows have been decoded (res[j]: the result of block blk[j] of a stream whose table is B): the length check of every block.
static inline void knz_read_settle_blocks(const int32_t* blk, int64_t cnt, const int64_t* B, int32_t nIndex, int32_t blockSize, kz_block_result* res) {
  for (int64_t j = 0; j < cnt; j++)
    if (!res[j].status) res[j].status = knz_block_len_check(B, nIndex, blockSize, blk[j], res[j].length);
}
// Behind it, the segments segs[s0 .. s1) of those rows (res[slot]) cut to what their blocks hold (a failed block's to nothing; unit0
// stays, the kernel skips the units that fall away), and got[]: the bytes delivered, or the status of the first failing block a range
// touches, in block order.
static inline void knz_read_settle_segs(KnzReadSeg* segs, int64_t s0, int64_t s1, const kz_block_result* res, int64_t* got) {
  for (int64_t i = s0; i < s1; i++) {
    KnzReadSeg& s = segs[i];
    const kz_block_result& r = res[s.slot];
    s.len = r.status ? 0 : (int32_t)std::max<int64_t>(0, std::min<int64_t>(s.len, (int64_t)r.length - s.off));
    if (got[s.range] < 0) continue;
    if (r.status) got[s.range] = r.status; else got[s.range] += s.len;
  }
}
// After chunk c has been decoded (res[j]: the result of its block j, rows of blockSize bytes): both steps.  got[] starts as zeros.
static inline void knz_read_settle(KnzReadPlan& P, int64_t c, int CH, const int64_t* B, int32_t nIndex, int32_t blockSize, kz_block_result* res, int64_t* got) {
  const int64_t b0 = c * CH, cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - b0);
  knz_read_settle_blocks(&P.blocks[(size_t)b0], cnt, B, nIndex, blockSize, res);
  knz_read_settle_segs(P.segs.data(), P.first[(size_t)c], P.first[(size_t)c + 1], res, got);
}

// ---- byte-addressed reads of many streams in one call (kz_read_bytes_many_device) ----
// Stream s is src[srcOff[s] .. + srcLen[s]) with the index entries [indexFirst[s], indexFirst[s + 1]) of blockBitOff / blockBits and,
// where tableFirst[s] >= 0, the table of block starts blockByteOff[tableFirst[s] ..] (its index length + 1 entries); range i asks
// stream rangeStream[i].  The arguments of the call, checked before anything else happens.
static inline int knz_many_src_args(const void* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams) {
  if (nStreams < 0 || (nStreams > 0 && (!src || !srcOff || !srcLen))) return -KZ_ERR_INVALID_PARAM;
  for (int32_t s = 0; s < nStreams; s++) if (srcOff[s] < 0 || srcLen[s] < 0) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
static inline int knz_read_many_args(const void* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams, const int64_t* indexFirst,
                                     const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* tableFirst, const int64_t* blockByteOff,
                                     const int32_t* rangeStream, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, const void* dst, int64_t dstCap,
                                     const int64_t* got) {
  if (nRanges < 0 || dstCap < 0) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_many_src_args(src, srcOff, srcLen, nStreams); if (rc) return rc; }
  if (nStreams > 0) {
    if (!indexFirst || indexFirst[0] < 0) return -KZ_ERR_INVALID_PARAM;
    for (int32_t s = 0; s < nStreams; s++)                         // ascending, and a stream's index has an int32 length as in the single call
      if (indexFirst[s + 1] < indexFirst[s] || indexFirst[s + 1] - indexFirst[s] > 0x7FFFFFFF) return -KZ_ERR_INVALID_PARAM;
    if (indexFirst[nStreams] > 0 && (!blockBitOff || !blockBits)) return -KZ_ERR_INVALID_PARAM;
    if (tableFirst)
      for (int32_t s = 0; s < nStreams; s++) if (tableFirst[s] < -1 || (tableFirst[s] >= 0 && !blockByteOff)) return -KZ_ERR_INVALID_PARAM;
  }
  if (nRanges > 0 && (!rangeStream || !rangeOff || !rangeLen || !dst || !got)) return -KZ_ERR_INVALID_PARAM;
  for (int32_t i = 0; i < nRanges; i++)
    if (rangeStream[i] < 0 || rangeStream[i] >= nStreams || rangeOff[i] < 0 || rangeLen[i] < 0) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
// What the plan needs to know of a stream: whether its ranges are read at all (a stream that no range names, or one with a fault of
// its own, is not), its header group (the streams with equal transform word, entropy id, block size and checksum kind, numbered in
// order of first appearance), its index length and block size, and its table of block starts (null: none).
struct KnzManyStreamIn { bool use; int32_t group; int32_t nIndex, blockSize; const int64_t* B; };
// The merged plan of the call: the distinct covering blocks of all streams that are read in one list of rows ordered by header group,
// then stream, then block; the rows cut into chunks, each inside one group and of at most that group's chunk size (chunkBlocks[g]
// >= 1); the range x block segments grouped by chunk as in KnzReadPlan, slot = the row's place in its chunk, dst = the range's place in
// the destination of the whole call (D[i] = the running sum of all requested lengths in call order).
struct KnzManyReadPlan {
  std::vector<int32_t> rowStream, rowBlock;   // the merged list
  std::vector<int64_t> chunkRow;              // chunk c = rows [chunkRow[c], chunkRow[c + 1])
  std::vector<int32_t> chunkGroup;            // its header group
  std::vector<KnzReadSeg> segs;               // chunk by chunk; inside a chunk by dst
  std::vector<int64_t> first;                 // chunk c owns segs[first[c] .. first[c + 1])
  std::vector<int64_t> units;                 // units[c] = the destination units of chunk c
};
static inline void knz_read_many_plan(const KnzManyStreamIn* st, int32_t nStreams, const int32_t* rangeStream, const int64_t* rangeOff, const int64_t* rangeLen,
                                      int32_t nRanges, const int* chunkBlocks, int dstPhase, KnzManyReadPlan& P) {
  (void)nStreams;
  P.rowStream.clear(); P.rowBlock.clear(); P.chunkGroup.clear();
  std::vector<KnzReadSeg> all;                                     // in range order: by dst
  std::vector<int32_t> blk, str;                                  // the block and the stream of all[i]
  int64_t D = 0;
  for (int32_t i = 0; i < nRanges; i++) {
    const int32_t s = rangeStream[i];
    const KnzManyStreamIn& S = st[s];
    if (S.use) {
      const int64_t end = S.B ? S.B[S.nIndex] : (int64_t)S.nIndex * S.blockSize;
      knz_read_cut(S.B, S.nIndex, S.blockSize, end, rangeOff[i], rangeLen[i], D, i, all, blk);
      str.resize(blk.size(), s);
    }
    D += rangeLen[i];                                              // (<= dstCap: knz_read_total)
  }
  struct Key { int32_t g, s, k; };
  auto less = [](const Key& a, const Key& b) { return a.g != b.g ? a.g < b.g : (a.s != b.s ? a.s < b.s : a.k < b.k); };
  std::vector<Key> rows(all.size());
  for (size_t i = 0; i < all.size(); i++) rows[i] = Key{st[str[i]].group, str[i], blk[i]};
  std::sort(rows.begin(), rows.end(), less);
  rows.erase(std::unique(rows.begin(), rows.end(), [](const Key& a, const Key& b) { return a.g == b.g && a.s == b.s && a.k == b.k; }), rows.end());
  std::vector<int64_t> rowChunk(rows.size());
  P.chunkRow.clear();
  for (size_t r = 0; r < rows.size(); r++) {
    P.rowStream.push_back(rows[r].s); P.rowBlock.push_back(rows[r].k);
    const bool open = !P.chunkGroup.empty() && P.chunkGroup.back() == rows[r].g && (int64_t)r - P.chunkRow.back() < chunkBlocks[rows[r].g];
    if (!open) { P.chunkRow.push_back((int64_t)r); P.chunkGroup.push_back(rows[r].g); }   // (a chunk never holds rows of two groups)
    rowChunk[r] = (int64_t)P.chunkGroup.size() - 1;
  }
  P.chunkRow.push_back((int64_t)rows.size());
  knz_read_split(all, (int64_t)P.chunkGroup.size(), dstPhase, [&](size_t i, int64_t& c, int32_t& slot) {
    const size_t r = (size_t)(std::lower_bound(rows.begin(), rows.end(), Key{st[str[i]].group, str[i], blk[i]}, less) - rows.begin());
    c = rowChunk[r]; slot = (int32_t)((int64_t)r - P.chunkRow[(size_t)c]);
  }, P.segs, P.first, P.units);
}

// ---- byte-addressed writes: many ranges of the original data replaced in one call (kz_write_bytes / kz_write_bytes_device) ----
// The plan of such a call, from host arrays alone, so that both forms share it.  Blocks and their starts B are the read's; range i
// brings data[D[i], D[i] + rangeLen[i]), D = the running sum of the lengths.  Ranges may overlap in any way and the later one in
// argument order wins: the plan turns them into disjoint SURVIVING segments, each one piece of one range cut with one block, so that
// every byte of the data has at most one segment (the last range that covers it) and the copy needs no order.  A range lies wholly
// inside the data, which is checked as len <= end - off before any off + len is formed: no int64 sum overflows.
struct KnzWriteSeg {         // 32 bytes: the entry of k_knz_write's table
  int64_t src;               // byte offset in data
  int64_t unit0;             // the segment's first 16-byte aligned row unit among the units of its chunk (prefix sum)
  int32_t slot;              // the block's row among the rows of its chunk
  int32_t off;               // byte offset in the block
  int32_t len;               // bytes (> 0)
  int32_t range;             // the owning range
};
struct KnzWritePlan {
  int64_t end;                         // the end of data as the arguments give it: B[nIndex], or nIndex * blockSize without a table
  std::vector<int32_t> blocks;         // the touched blocks, ascending; chunk c = blocks[c * CH .. (c + 1) * CH)
  std::vector<uint8_t> covered;        // covered[i]: blocks[i] is wholly overwritten and a table gave its length: no decode, no check
  std::vector<KnzWriteSeg> segs;       // ascending by place in the data, that is by block and by offset in it: chunk by chunk
  std::vector<int64_t> first;          // chunk c owns segs[first[c] .. first[c + 1])
  std::vector<int64_t> units;          // units[c] = the row units of chunk c: what unit0 sums up to
  std::vector<int64_t> cuts;           // launch l copies segs[cuts[l] .. cuts[l + 1]): at most `launch` segments, of one chunk
};
// dataLen == D[nRanges] included; newBitOff / newBits: both or neither
static inline int knz_write_args(const void* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nIndex, const int64_t* rangeOff,
                                 const int64_t* rangeLen, int32_t nRanges, const void* data, int64_t dataLen, const void* dst, int64_t dstCap,
                                 const int64_t* newBitOff, const int64_t* newBits) {
  if (!src || n < 0 || nIndex < 0 || nRanges < 0 || dataLen < 0 || !dst || dstCap < 0 || (nIndex > 0 && (!blockBitOff || !blockBits))) return -KZ_ERR_INVALID_PARAM;
  if ((nRanges > 0 && (!rangeOff || !rangeLen)) || (dataLen > 0 && !data) || (!newBitOff != !newBits)) return -KZ_ERR_INVALID_PARAM;
  int64_t D = 0;
  for (int32_t i = 0; i < nRanges; i++) {
    if (rangeOff[i] < 0 || rangeLen[i] < 0 || rangeLen[i] > dataLen - D) return -KZ_ERR_INVALID_PARAM;
    D += rangeLen[i];
  }
  return D == dataLen ? 0 : -KZ_ERR_INVALID_PARAM;
}
// kz_write_bytes_bound: the longest stream header, per block 5 + 34 prefix bits and the longer of its own payload and a recoded
// block's bound, the end marker
static inline int64_t knz_write_bound(const int64_t* blockBits, int32_t nIndex, int32_t blockSize) {
  if (nIndex < 0 || (nIndex > 0 && !blockBits) || !knz_block_size_ok(blockSize)) return -KZ_ERR_INVALID_PARAM;
  const int64_t rec = 8 * (((int64_t)blockSize + (blockSize >> 3) + 1024 + 255) / 256 * 256);   // kz_max_block_stream_bytes, restated: no library here
  int64_t bits = 8;
  for (int32_t k = 0; k < nIndex; k++) {
    if (blockBits[k] < 0 || blockBits[k] >= (1LL << 34)) return -KZ_ERR_INVALID_PARAM;
    bits += 5 + 34 + std::max<int64_t>(blockBits[k], rec);
    if (bits > (1LL << 62)) return -KZ_ERR_INVALID_PARAM;
  }
  return 26 + ((bits + 7) >> 3);
}
static inline int knz_write_behind(int32_t i, char* err, size_t errCap) {
  if (err) snprintf(err, errCap, "range %d ends behind the data", (int)i);
  return -KZ_ERR_INVALID_PARAM;
}
// The plan.  The arguments have passed knz_write_args and knz_read_table; CH >= 1 = touched blocks per chunk, launch >= 1 = segments
// per launch.  Returns -1, or the first range that ends behind P.end (nothing else of P is then filled).
// Later wins by a sort and a sweep, O(nRanges log nRanges): the ranges' starts and ends in ascending order cut the data into at most
// 2 nRanges elementary intervals; over each the owner is the highest range among those open there (a heap of the open ranges, closed
// ones dropped when they come to the top).  Neighbours of one owner are joined, then each piece is cut with the blocks.
// knz_write_plan_at is the form for a call whose new bytes are packed over the ranges of many streams (kz_write_bytes_many_device): range
// i brings data[rangeData[i] .. + rangeLen[i]); null = the running sum, the single-stream calls' rule.
static inline int32_t knz_write_plan_at(const int64_t* B, int32_t nIndex, int32_t blockSize, const int64_t* rangeOff, const int64_t* rangeLen, const int64_t* rangeData,
                                        int32_t nRanges, int CH, int64_t launch, KnzWritePlan& P) {
  P.end = B ? B[nIndex] : (int64_t)nIndex * blockSize;
  P.blocks.clear(); P.covered.clear(); P.segs.clear(); P.first.assign(1, 0); P.units.clear(); P.cuts.assign(1, 0);
  std::vector<int64_t> D((size_t)nRanges + 1, 0);
  int64_t run = 0;                                                 // the running sum of the lengths
  std::vector<int32_t> open;                                       // the ranges with bytes, by start (ties: by argument order)
  std::vector<int64_t> pts;
  for (int32_t i = 0; i < nRanges; i++) {
    if (rangeOff[i] > P.end || rangeLen[i] > P.end - rangeOff[i]) return i;
    D[(size_t)i] = rangeData ? rangeData[i] : run;
    run += rangeLen[i];
    if (rangeLen[i] == 0) continue;
    open.push_back(i);
    pts.push_back(rangeOff[i]); pts.push_back(rangeOff[i] + rangeLen[i]);          // (<= P.end: checked above)
  }
  std::sort(open.begin(), open.end(), [&](int32_t a, int32_t b) { return rangeOff[a] != rangeOff[b] ? rangeOff[a] < rangeOff[b] : a < b; });
  std::sort(pts.begin(), pts.end());
  pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
  struct Piece { int64_t at, len; int32_t range; };
  std::vector<Piece> pieces;
  {
    std::vector<int32_t> heap;                                     // max-heap of range numbers
    size_t nx = 0;
    for (size_t p = 0; p + 1 < pts.size(); p++) {
      const int64_t a = pts[p], b = pts[p + 1];
      while (nx < open.size() && rangeOff[open[nx]] == a) { heap.push_back(open[nx++]); std::push_heap(heap.begin(), heap.end()); }
      while (!heap.empty() && rangeOff[heap.front()] + rangeLen[heap.front()] <= a) { std::pop_heap(heap.begin(), heap.end()); heap.pop_back(); }
      if (heap.empty()) continue;
      const int32_t r = heap.front();
      if (!pieces.empty() && pieces.back().range == r && pieces.back().at + pieces.back().len == a) pieces.back().len += b - a;
      else pieces.push_back(Piece{a, b - a, r});
    }
  }
  std::vector<int32_t> blk;                                        // the block of segs[i]
  std::vector<int64_t> have;                                       // surviving bytes per touched block
  for (const Piece& pc : pieces) {
    int64_t src = D[(size_t)pc.range] + (pc.at - rangeOff[pc.range]);
    knz_cut_at_blocks(B, blockSize, knz_block_of(B, nIndex, blockSize, pc.at), pc.at, pc.len, [&](int64_t k, int64_t off, int64_t len) {
      if (P.blocks.empty() || P.blocks.back() != (int32_t)k) { P.blocks.push_back((int32_t)k); have.push_back(0); }
      have.back() += len;
      P.segs.push_back(KnzWriteSeg{src, 0, (int32_t)((int64_t)(P.blocks.size() - 1) % CH), (int32_t)off, (int32_t)len, pc.range});
      blk.push_back((int32_t)(P.blocks.size() - 1));
      src += len;
    });
  }
  P.covered.resize(P.blocks.size());
  for (size_t i = 0; i < P.blocks.size(); i++) P.covered[i] = (B && have[i] == B[P.blocks[i] + 1] - B[P.blocks[i]]) ? 1 : 0;
  const int64_t nChunks = ((int64_t)P.blocks.size() + CH - 1) / CH;
  P.first.assign((size_t)nChunks + 1, 0);
  P.units.assign((size_t)nChunks, 0);
  for (size_t i = 0; i < P.segs.size(); i++) {                     // (already chunk by chunk: blocks ascend with the segments)
    const int64_t c = blk[i] / CH;
    P.first[(size_t)c + 1] = (int64_t)i + 1;
    P.segs[i].unit0 = P.units[(size_t)c];
    P.units[(size_t)c] += knz_read_units(P.segs[i].off & 15, P.segs[i].len);       // rows start on a 16-byte boundary, blockSize apart
  }
  for (int64_t c = 0; c < nChunks; c++)
    for (int64_t s = P.first[(size_t)c]; s < P.first[(size_t)c + 1];) {
      s += std::min<int64_t>(launch, P.first[(size_t)c + 1] - s);
      P.cuts.push_back(s);
    }
  return -1;
}
static inline int32_t knz_write_plan(const int64_t* B, int32_t nIndex, int32_t blockSize, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                                     int CH, int64_t launch, KnzWritePlan& P) {
  return knz_write_plan_at(B, nIndex, blockSize, rangeOff, rangeLen, nullptr, nRanges, CH, launch, P);
}
// The results of the wholly covered blocks among blocks[b0 .. b0 + cnt), which are not decoded: before the chunk's decode status 1
// (left out of it), behind it (decoded) status 0 and the table's length, as if they had been.
static inline void knz_write_covered(const KnzWritePlan& P, int64_t b0, int cnt, const int64_t* B, bool decoded, kz_block_result* res) {
  for (int i = 0; i < cnt; i++) {
    if (!P.covered[(size_t)(b0 + i)]) continue;
    const int32_t k = P.blocks[(size_t)(b0 + i)];
    memset(&res[i], 0, sizeof(res[i]));
    if (decoded) res[i].length = (int32_t)(B[k + 1] - B[k]); else res[i].status = 1;
  }
}
// After chunk c has been decoded (res[j]: the result of its block j; the caller gave a wholly covered block status 0 and the table's
// length): the length check of every block as knz_read_settle makes it, and, without a table, the segments against the real end of a
// short last block.  lens[j] = the bytes of row j when the chunk is patched.  Returns 0, or the code of the first failing block in
// block order with its text in err ("block %d: ..."; a range across the end of the last block: knz_write_behind's).
static inline int knz_write_settle(const KnzWritePlan& P, int64_t c, int CH, const int64_t* B, int32_t nIndex, int32_t blockSize, kz_block_result* res, int32_t* lens,
                                   char* err, size_t errCap) {
  const int64_t b0 = c * CH, cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - b0);
  for (int64_t j = 0; j < cnt; j++) {
    const int32_t k = P.blocks[(size_t)(b0 + j)];
    const char* why = "its decode failed";
    if (!res[j].status) {
      res[j].status = knz_block_len_check(B, nIndex, blockSize, k, res[j].length);
      why = res[j].status == -KZ_ERR_PROCESS_BLOCK ? "decodes to more than the block size" : "decodes to another length than its place in the data";
    }
    if (res[j].status) {
      if (err) snprintf(err, errCap, "block %d: %s (%d)", (int)k, why, (int)res[j].status);
      return res[j].status;
    }
    lens[j] = res[j].length;
  }
  if (!B)
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzWriteSeg& s = P.segs[(size_t)i];
      if ((int64_t)s.off + s.len > lens[s.slot]) return knz_write_behind(s.range, err, errCap);
    }
  return 0;
}
// The layout of blocks [k0, k1) of the rewritten stream from bit `pos` on.  touched = the plan's blocks (ascending), t = the first of
// them at or behind k0 (it moves on with the walk), t1 = the end of those that are recoded here; eW[0 ..] = the recoded blocks' bits
// from touched[t] on.  Every other block keeps its blockBits[k].  Per block, block(k, r, W, pay): r = its place in touched when it is
// recoded, else -1; W = its bits; pay = the bit where its payload starts, behind its 5 + lw prefix bits.  Returns the bit behind the
// last block: with a callback that does nothing this is the room decision, made before a bit is written.
template <class F> static inline int64_t knz_write_walk(const int64_t* blockBits, const int32_t* touched, int64_t k0, int64_t k1, int64_t& t, int64_t t1,
                                                        const int64_t* eW, int64_t pos, F block) {
  const int64_t tb = t;
  for (int64_t k = k0; k < k1; k++) {
    const bool rec = t < t1 && touched[t] == k;
    const int64_t W = rec ? eW[t - tb] : blockBits[k];
    pos += 5 + knz_prefix_width((uint64_t)W);
    block(k, rec ? t++ : (int64_t)-1, W, pos);
    pos += W;
  }
  return pos;
}
static inline void knz_write_walk_only(int64_t, int64_t, int64_t, int64_t) {}

// ---- byte-addressed writes of many streams in one call (kz_write_bytes_many_device) ----
// Streams, indices, tables and ranges are the many-stream read's; slots are kz_compress_many_device's; the new bytes are packed over
// all ranges in call order.  The arguments of the call, checked before anything else happens.
static inline int knz_write_many_args(const void* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams, const int64_t* indexFirst,
                                      const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* tableFirst, const int64_t* blockByteOff,
                                      const int32_t* rangeStream, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, const void* data, int64_t dataLen,
                                      const void* dst, const int64_t* dstOff, const int64_t* dstCap, const int64_t* dstLen, const int64_t* newBitOff, const int64_t* newBits) {
  if (nRanges < 0 || dataLen < 0 || (!newBitOff != !newBits)) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_many_src_args(src, srcOff, srcLen, nStreams); if (rc) return rc; }
  if (nStreams > 0) {
    if (!indexFirst || indexFirst[0] < 0 || !dst || !dstOff || !dstCap || !dstLen) return -KZ_ERR_INVALID_PARAM;
    for (int32_t s = 0; s < nStreams; s++)
      if (indexFirst[s + 1] < indexFirst[s] || indexFirst[s + 1] - indexFirst[s] > 0x7FFFFFFF || dstOff[s] < 0 || dstCap[s] < 0) return -KZ_ERR_INVALID_PARAM;
    if (indexFirst[nStreams] > 0 && (!blockBitOff || !blockBits)) return -KZ_ERR_INVALID_PARAM;
    if (tableFirst)
      for (int32_t s = 0; s < nStreams; s++) if (tableFirst[s] < -1 || (tableFirst[s] >= 0 && !blockByteOff)) return -KZ_ERR_INVALID_PARAM;
  }
  if ((nRanges > 0 && (!rangeStream || !rangeOff || !rangeLen)) || (dataLen > 0 && !data)) return -KZ_ERR_INVALID_PARAM;
  int64_t D = 0;
  for (int32_t i = 0; i < nRanges; i++) {
    if (rangeStream[i] < 0 || rangeStream[i] >= nStreams || rangeOff[i] < 0 || rangeLen[i] < 0 || rangeLen[i] > dataLen - D) return -KZ_ERR_INVALID_PARAM;
    D += rangeLen[i];
  }
  return D == dataLen ? 0 : -KZ_ERR_INVALID_PARAM;
}
// kz_write_bytes_many_bound: knz_write_bound of every stream's entries and block size, and their sum
static inline int64_t knz_write_many_bound(const int64_t* indexFirst, const int64_t* blockBits, const int32_t* blockSize, int32_t nStreams, int64_t* slotCap) {
  if (nStreams < 0 || (nStreams > 0 && (!indexFirst || !blockSize || indexFirst[0] < 0))) return -KZ_ERR_INVALID_PARAM;
  int64_t sum = 0;
  for (int32_t s = 0; s < nStreams; s++) {
    const int64_t cnt = indexFirst[s + 1] - indexFirst[s];
    if (cnt < 0 || cnt > 0x7FFFFFFF || (cnt > 0 && !blockBits)) return -KZ_ERR_INVALID_PARAM;
    const int64_t cap = knz_write_bound(cnt ? blockBits + indexFirst[s] : nullptr, (int32_t)cnt, blockSize[s]);
    if (cap < 0) return cap;
    if (slotCap) slotCap[s] = cap;
    sum += cap;
    if (sum > (1LL << 62)) return -KZ_ERR_INVALID_PARAM;
  }
  return sum;
}
// What the merged plan needs to know of a stream: whether it is written at all (a stream that no range names, or one with a fault of
// its own, is not), its header group as in KnzManyStreamIn, its own plan (knz_write_plan_at with one chunk: a segment's slot is its
// block's place among the stream's touched blocks) and the number in the call of each of its ranges.
struct KnzManyWriteIn { bool use; int32_t group; const KnzWritePlan* plan; const int32_t* rangeId; };
// The merged plan of the call: the touched blocks of all streams that are written, covered ones included, in one list of rows ordered
// by header group, then stream, then block; the rows cut into chunks, each inside one group and of at most that group's chunk size
// (knz_read_many_plan's rule); the surviving segments of all streams chunk by chunk in row order, as KnzWritePlan holds them: slot = the
// row's place in its chunk, unit0 = the prefix sum of the row units inside the chunk, range = the range's number in the call, cuts =
// the patch launches.  A written stream with no touched block has no row.
struct KnzManyWritePlan {
  std::vector<int32_t> rowStream, rowBlock;   // the merged list
  std::vector<uint8_t> rowCovered;            // the row's block is wholly overwritten and a table gave its length
  std::vector<int64_t> chunkRow;              // chunk c = rows [chunkRow[c], chunkRow[c + 1])
  std::vector<int32_t> chunkGroup;            // its header group
  std::vector<KnzWriteSeg> segs;              // chunk by chunk; inside a chunk by row, then by offset in the block
  std::vector<int64_t> first, units, cuts;    // as in KnzWritePlan
};
static inline void knz_write_many_plan(const KnzManyWriteIn* st, int32_t nStreams, const int* chunkBlocks, int64_t launch, KnzManyWritePlan& P) {
  P.rowStream.clear(); P.rowBlock.clear(); P.rowCovered.clear(); P.chunkRow.clear(); P.chunkGroup.clear();
  P.segs.clear(); P.first.assign(1, 0); P.units.clear(); P.cuts.assign(1, 0);
  std::vector<int32_t> order;
  for (int32_t s = 0; s < nStreams; s++) if (st[s].use && !st[s].plan->blocks.empty()) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return st[a].group < st[b].group; });   // (inside a group: by stream)
  for (const int32_t s : order) {
    const KnzWritePlan& W = *st[s].plan;
    const int32_t g = st[s].group;
    size_t si = 0;                                                 // the stream's next segment: they ascend with its blocks
    for (size_t t = 0; t < W.blocks.size(); t++) {
      const int64_t r = (int64_t)P.rowStream.size();
      const bool open = !P.chunkGroup.empty() && P.chunkGroup.back() == g && r - P.chunkRow.back() < chunkBlocks[g];
      if (!open) {                                                 // (a chunk never holds rows of two groups)
        if (!P.chunkGroup.empty()) P.first.push_back((int64_t)P.segs.size());
        P.chunkRow.push_back(r); P.chunkGroup.push_back(g); P.units.push_back(0);
      }
      P.rowStream.push_back(s); P.rowBlock.push_back(W.blocks[t]); P.rowCovered.push_back(W.covered[t]);
      for (; si < W.segs.size() && W.segs[si].slot == (int32_t)t; si++) {
        KnzWriteSeg q = W.segs[si];
        q.slot = (int32_t)(r - P.chunkRow.back());
        q.unit0 = P.units.back();
        q.range = st[s].rangeId[q.range];
        P.units.back() += knz_read_units(q.off & 15, q.len);
        P.segs.push_back(q);
      }
    }
  }
  if (!P.chunkGroup.empty()) P.first.push_back((int64_t)P.segs.size());
  P.chunkRow.push_back((int64_t)P.rowStream.size());
  for (size_t c = 0; c + 1 < P.first.size(); c++)
    for (int64_t s = P.first[c]; s < P.first[c + 1];) {
      s += std::min<int64_t>(launch, P.first[c + 1] - s);
      P.cuts.push_back(s);
    }
}
