// kz_exe.hip -- EXE, the x86 / ARM64 branch-address transform (K/transform/EXECodec.java, bitstream >= 3): forward and inverse on the
// device, batched (grid.y = block), tile-parallel inside a block.  tests/exemodel.py restates the Java and is the contract.
//
// What a byte means depends on the bytes before it only through a small state: "bytes still owed to the current instruction" and
// "second byte of 0F" (x86 forward), the same plus "byte after a 9B" (x86 inverse), "bytes owed to the current word or escape pair"
// (ARM64 inverse), "bytes the heuristic's 0F arm still skips" (detectType).  The ARM64 forward has no state: every word from codeStart
// on stands alone.  All five are run by the same passes, as the RLT inverse is (kz_rlt.hip): a thread takes EX_PER consecutive bytes
// and composes their transition maps (8 states x 4 bits in a word), a wave scan and LDS give the map of a tile of EX_TILE bytes
// (k_exe_map), one wave per block composes the tiles' maps into the state at every tile's start (k_exe_scan).  With the states known a
// thread walks its bytes as the reference does: output sizes, the match count and the failures (k_exe_size), offsets by sum-scan and
// the block's verdict (k_exe_verdict), then the bytes (k_exe_emit).  An address needs only the position of its opcode byte (forward:
// in the source; inverse: in the output, which is the thread's offset), so the emit pass is independent per instruction.  No
// workgroup waits for another inside a kernel.
//
// FORWARD.  k_exe_setup (one lane per block) applies the size and data-type rules (:119, :130-137) and parseHeader (:802-1011): a few
// dozen dependent loads, each checked against the block (no block of 4 096 bytes and more reaches a read past its end: every offset
// is compared with `count` first).  A block whose header does not name a known architecture goes through the heuristic (:701-772):
// k_exe_map / k_exe_scan run the skip automaton (a visited 0F jumps over one or two bytes, which are neither counted nor tested),
// k_exe_hist counts the visited bytes and the two kinds of jumps, k_exe_decide applies detectSimpleType and the thresholds.  The
// verdict (matches >= 16, total <= count + count / 50) is known before a byte of dst is written: a declined block leaves dst alone.
//
// dst.length: the reference's loops also stop at dstIdx >= dstEnd (dst.length - 5, ARM64: - 8).  For every dst.length >=
// getMaxEncodedLength(count) -- smaller ones are declined up front (:127, transform_one) -- a loop stopped that way has passed
// count + count / 50 already (count / 8 - 8 > count / 50 from 4 096 on) and the block is declined either way, so the batched forward
// needs no per-block dst.length as RLT's does.
//
// INVERSE.  k_exe_setup checks the header (:390-401, :413-415); the passes run on the coded bytes; every store is below the block's
// decoded length, which k_exe_verdict has compared with dstCap (the reference checks per store and fails at the first one that does
// not fit: the same verdict, since the output only grows).
#include "kz_device.h"
#include "kz_internal.h"
#include "kz_datatype.h"
#include "kz_magic.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

#define EX_PER 16                          // bytes per thread strip
#define EX_TILE (KZ_WG * EX_PER)           // bytes per workgroup
#define EX_IDENT 0x76543210u
enum { EX_NONE = 0, EX_DET = 1, EX_X86F = 2, EX_ARMF = 3, EX_X86I = 4, EX_ARMI = 5 };
enum { EXF_MATCH = 1, EXF_FAIL = 2, EXF_EXIT = 4, EXF_ESC = 8 };
#define EX_MODE_X86 0x40                   // :43
#define EX_MODE_ARM64 0x20                 // :44
#define EX_MIN_BLOCK 4096                  // :71
#define EX_MAX_BLOCK ((1 << 28) - 1)       // :72
#define EX_MASK_ADDRESS 0xF0F0F0F0u        // :47
#define EX_ARM_OPMASK 0xFC000000u          // :49
#define EX_ARM_ADDRMASK 0x03FFFFFFu        // :48
#define EX_ARM_B 0x14000000u               // :51
#define EX_ARM_BL 0x94000000u              // :52

struct ExScratch {
  int T;             // tiles per block (+1)
  u32* tMap;         // [B][T] transition map of the tile
  u32* tState;       // [B][T] state at the tile's first byte
  u32* tSum;         // [B][T] output bytes of the tile
  u32* tOff;         // [B][T] output offset of the tile
  uint16_t* strip;   // [B][T * KZ_WG] per thread strip: entry state | output bytes << 4
  u32* hist;         // [B][256] the heuristic's histogram of visited bytes
  int4* info;        // [B] mode (EX_*), first and end position of the state machine, block length
  int32_t* jumps;    // [B][2] the heuristic's x86 / ARM64 jump counts
  int32_t* matches;  // [B]
  int32_t* fail;     // [B]
  int32_t* exitPos;  // [B] forward: where the tail copy starts (a boundary exit, else codeEnd; ARM64: behind the last whole word)
  int32_t* cstart;   // [B] forward: codeStart for the header
};

__host__ __device__ __forceinline__ u32 ex_nib(u32 m, u32 s) { return (m >> (4u * s)) & 7u; }
// first a, then b
__host__ __device__ __forceinline__ u32 ex_compose(u32 a, u32 b) {
  u32 r = 0;
#pragma unroll
  for (int s = 0; s < 8; s++) r |= ex_nib(b, ex_nib(a, (u32)s)) << (4 * s);
  return r;
}

// the thread's 16 bytes and the 8 behind them (the slack behind every block of a batch is 4 096 bytes); bytes at and behind n read 0
__host__ __device__ __forceinline__ void ex_load(const u8* __restrict__ s, int pos, int n, u64 q[3]) {
  q[0] = q[1] = q[2] = 0;
  if (pos < n) {
    const uint4 v = *(const uint4*)(s + pos);
    const uint2 l = *(const uint2*)(s + pos + 16);
    q[0] = (u64)v.x | ((u64)v.y << 32); q[1] = (u64)v.z | ((u64)v.w << 32); q[2] = (u64)l.x | ((u64)l.y << 32);
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int base = pos + 8 * j;
    if (base >= n) q[j] = 0;
    else if (base + 8 > n) q[j] &= (1ULL << (8 * (n - base))) - 1ULL;
  }
}
// bytes p .. p + 7 of the strip's position k
__host__ __device__ __forceinline__ u64 ex_win(const u64 q[3], int k) {
  const int j = k >> 3, sh = (k & 7) * 8;
  u64 w = q[j] >> sh;
  if (sh) w |= q[j + 1] << (64 - sh);
  return w;
}

struct ExStep { u32 next, sz, flags; };

// one byte of the reference's loops: the state behind position p, the output bytes the position accounts for (an instruction's bytes
// are all counted at its opcode byte, a word's at its first byte) and what happened.  lo / hi: where the state machine runs.
__host__ __device__ __forceinline__ ExStep ex_step(int mode, u32 st, int p, u64 win, int lo, int hi, int n) {
  ExStep r; r.next = st; r.sz = 1; r.flags = 0;                    // a byte copied as it is
  if (p >= n) { r.sz = 0; return r; }
  const u32 b0 = (u32)win & 0xFFu, b1 = (u32)(win >> 8) & 0xFFu, b4 = (u32)(win >> 32) & 0xFFu;
  if (mode == EX_DET) {                                            // :706-734
    r.sz = 0;
    if (st) { r.next = (st <= 2u) ? st - 1u : st; return r; }
    // the E8 / E9 test comes first (:710); a byte cannot be both
    if (b0 == 0x0Fu && p + 1 < n) r.next = ((b1 == 0x38u || b1 == 0x3Au) && p + 2 < n) ? 2u : 1u;
    return r;
  }
  if (mode == EX_X86F) {                                           // :183-242
    if (p < lo || p >= hi || st >= 6u) return r;
    if (st >= 1u && st <= 4u) { r.next = st - 1u; r.sz = 0; return r; }
    if (st == 0u) {
      if (b0 == 0x0Fu) {
        if (p + 1 >= hi || ((b1 & 0xF0u) == 0x80u && p + 5 >= hi)) { r.next = 6u; r.flags = EXF_EXIT; return r; }   // :185, :190-195
        r.next = 5u; return r;
      }
      if ((b0 & 0xFEu) != 0xE8u) { r.sz = 1u + (b0 == 0x9Bu); return r; }                                            // :212-218
      if (p + 4 >= hi) { r.next = 6u; r.flags = EXF_EXIT; return r; }                                                // :219
    } else if ((b0 & 0xF0u) != 0x80u) { r.next = 0u; r.sz = 1u + (b0 == 0x9Bu); return r; }                           // :199-206
    const u32 off = (u32)(win >> 8);
    if ((b4 != 0u && b4 != 0xFFu) || off == 0xFF000000u) { r.next = 0u; r.sz = 2; return r; }                         // :229-233
    r.next = 4u; r.sz = 5; r.flags = EXF_MATCH; return r;
  }
  if (mode == EX_ARMF) {                                           // :281-341; hi: behind the last whole word
    if (p < lo || p >= hi) return r;
    r.sz = 0;
    if ((p - lo) & 3) return r;
    const u32 instr = (u32)win, op1 = instr & EX_ARM_OPMASK;
    r.sz = 4;
    if (op1 != EX_ARM_B && op1 != EX_ARM_BL) return r;
    int addr = p + 4 * (((int32_t)(instr << 6)) >> 6);             // :307
    if (addr < 0) addr = 0;
    if (addr == 0) { r.sz = 8; r.flags = EXF_ESC; } else r.flags = EXF_MATCH;
    return r;
  }
  // the two inverses: the 9 header bytes produce nothing
  if (p < 9) { r.sz = 0; return r; }
  if (p < lo || p >= hi) return r;
  if (mode == EX_X86I) {                                           // :423-485
    if (st >= 1u && st <= 4u) { r.next = st - 1u; r.sz = 0; return r; }
    if (st == 6u) { r.next = 0u; return r; }                       // the byte behind a 9B, whatever it is
    if (st == 7u) return r;
    if (st == 0u && b0 == 0x0Fu) { r.next = 5u; return r; }        // (a trailing 0F at codeEnd - 1 included, :425-433)
    const bool jump = (st == 0u) ? ((b0 & 0xFEu) == 0xE8u) : ((b0 & 0xF0u) == 0x80u);
    if (!jump) {
      r.next = 0u;
      if (b0 == 0x9Bu) { r.next = 6u; r.sz = 0; if (p + 1 >= hi) r.flags = EXF_FAIL; }        // :442-447, :457-462
      return r;
    }
    r.next = 4u; r.sz = 5; r.flags = EXF_MATCH | ((p + 4 >= hi) ? EXF_FAIL : 0);               // :471
    return r;
  }
  // EX_ARMI, :580-634
  r.sz = 0;
  if (st) { r.next = st - 1u; return r; }
  if (p + 4 > hi) { r.flags = EXF_FAIL; return r; }                // :581
  const u32 instr = (u32)win, op1 = instr & EX_ARM_OPMASK;
  r.sz = 4; r.next = 3u;
  if (op1 != EX_ARM_B && op1 != EX_ARM_BL) return r;
  if ((instr & EX_ARM_ADDRMASK) == 0u) { r.next = 7u; r.flags = EXF_ESC | ((p + 8 > hi) ? EXF_FAIL : 0); }   // :618-629
  else r.flags = EXF_MATCH;
  return r;
}

// the transition map of one position: only "instruction start" and "behind 0F" look at the byte
__host__ __device__ __forceinline__ u32 ex_pos_map(int mode, int p, u64 win, int lo, int hi, int n) {
  if (p >= n || mode == EX_ARMF) return EX_IDENT;
  const u32 t0 = ex_step(mode, 0u, p, win, lo, hi, n).next;
  if (mode == EX_DET) return 0x76543100u | t0;
  if (p < lo || p >= hi || p < ((mode >= EX_X86I) ? 9 : 0)) return EX_IDENT;
  if (mode == EX_ARMI) return 0x65432100u | t0;
  const u32 t5 = ex_step(mode, 5u, p, win, lo, hi, n).next;
  return ((mode == EX_X86F) ? 0x76032100u : 0x70032100u) | t0 | (t5 << 20);
}

__host__ __device__ __forceinline__ u32 ex_thread_map(int mode, const u64 q[3], int pos, int lo, int hi, int n) {
  u32 m = EX_IDENT;
#pragma unroll
  for (int k = 0; k < EX_PER; k++) m = ex_compose(m, ex_pos_map(mode, pos + k, ex_win(q, k), lo, hi, n));
  return m;
}

// the composition of the maps of the threads before this one; *total: of the whole workgroup.  ldsm: KZ_WG / 64 words
__device__ __forceinline__ u32 ex_wg_excl_map(u32 m, u32* ldsm, u32* total) {
  const int lane = kz_lane(), wave = (int)threadIdx.x >> 6;
  u32 inc = m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if (lane >= d) inc = ex_compose(up, inc); }
  u32 ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = EX_IDENT;
  __syncthreads();
  if (lane == 63) ldsm[wave] = inc;
  __syncthreads();
  u32 pre = EX_IDENT, tot = EX_IDENT;
  for (int w = 0; w < KZ_WG / 64; w++) { if (w < wave) pre = ex_compose(pre, ldsm[w]); tot = ex_compose(tot, ldsm[w]); }
  *total = tot;
  return ex_compose(pre, ex);
}

// ---- parseHeader (:784-1011), one lane ------------------------------------------------------------------------------------------------
struct ExHdr { int cs, ce, arch; const u8* s; int count; bool past; };
__host__ __device__ __forceinline__ u64 ex_rd(ExHdr& H, long long off, int k, bool big) {
  if (off < 0 || off + k > (long long)H.count) { H.past = true; return 0; }      // the Java would throw
  u64 v = 0;
  for (int i = 0; i < k; i++) v |= (u64)H.s[off + i] << (big ? 8 * (k - 1 - i) : 8 * i);
  return v;
}
__host__ __device__ __forceinline__ bool ex_set_range(ExHdr& H, long long rs, long long rl, bool updateStart) {     // :784-800 with start = 0
  if (rs < 0 || rl < 0 || rs > H.count || rl > (long long)H.count - rs) return false;
  if (updateStart || H.cs == 0) H.cs = (int)rs;
  H.ce = (int)(rs + rl);
  return true;
}
__host__ __device__ inline bool ex_parse_header(ExHdr& H) {
  const int count = H.count;
  const int32_t magic = mm_magic_type(H.s);
  if (count < 64) return false;
  if (magic == 0x4D5A) {                                                         // :803-819
    H.arch = (int)(u32)ex_rd(H, 18, 4, false);
    const int posPE = (int)(u32)ex_rd(H, 60, 4, false);
    if (posPE > 0 && posPE <= count - 48 && (u32)ex_rd(H, posPE, 4, false) == 0x00004550u) {
      if (!ex_set_range(H, (int)(u32)ex_rd(H, posPE + 44, 4, false), (int)(u32)ex_rd(H, posPE + 28, 4, false), true)) return false;
      H.arch = (int)ex_rd(H, posPE + 4, 2, false);
    }
    return !H.past;
  }
  if ((u32)magic == 0x7F454C46u) {                                               // :820-936
    const bool big = H.s[5] != 1, is64 = H.s[4] == 2;
    H.cs = 0;
    const int nb = (int)ex_rd(H, is64 ? 0x3C : 0x30, 2, big), sz = (int)ex_rd(H, is64 ? 0x3A : 0x2E, 2, big);
    const long long pos = is64 ? (long long)ex_rd(H, 0x28, 8, big) : (long long)(int)(u32)ex_rd(H, 0x20, 4, big);
    const int room = is64 ? 0x28 : 0x18;
    if (sz <= 0 || pos < 0 || pos > (long long)count - room) return false;
    for (int i = 0; i < nb; i++) {
      const long long e = pos + (long long)i * sz;
      if (e < 0 || e > (long long)count - room) return false;
      const int typ = (int)(u32)ex_rd(H, e + 4, 4, big);
      const long long off = is64 ? (long long)ex_rd(H, e + 0x18, 8, big) : (long long)(int)(u32)ex_rd(H, e + 0x10, 4, big);
      const long long len = is64 ? (long long)ex_rd(H, e + 0x20, 8, big) : (long long)(int)(u32)ex_rd(H, e + 0x14, 4, big);
      if (H.past) return false;
      if (typ == 1 && len >= 64 && !ex_set_range(H, off, len, false)) return false;
    }
    H.arch = (int)ex_rd(H, 18, 2, false);                                        // :932: little-endian whatever the file says
    if (H.cs > count) H.cs = count;
    if (H.ce > count) H.ce = count;
    return !H.past;
  }
  const u32 k = (u32)magic;
  if (k == 0xFEEDFACEu || k == 0xCEFAEDFEu || k == 0xFEEDFACFu || k == 0xCFFAEDFEu) {      // :937-1007
    const bool is64 = k == 0xFEEDFACFu || k == 0xCFFAEDFEu;
    H.cs = 0;
    if ((int)(u32)ex_rd(H, 12, 4, false) != 0x02) return false;                  // MH_EXECUTE only
    H.arch = (int)(u32)ex_rd(H, 4, 4, false);
    const int nbCmds = (int)(u32)ex_rd(H, 0x10, 4, false);
    int pos = is64 ? 0x20 : 0x1C;
    const int szSeg = is64 ? 0x48 : 0x38;
    for (int cmd = 0; cmd < nbCmds; cmd++) {
      if (pos > count - 8) return false;
      const int ldCmd = (int)(u32)ex_rd(H, pos, 4, false), szCmd = (int)(u32)ex_rd(H, pos + 4, 4, false);
      if (szCmd < 8 || szCmd > count - pos) return false;
      if (ldCmd == 0x01 || ldCmd == 0x19) {
        if (pos > count - 14 || pos > count - szSeg) return false;
        if ((ex_rd(H, pos + 8, 8, true) >> 16) == 0x5F5F54455854ULL) {           // "__TEXT"
          const int posSec = pos + szSeg;
          if (posSec > count - (is64 ? 0x38 : 0x30)) return false;
          if ((ex_rd(H, posSec, 8, true) >> 16) == 0x5F5F74657874ULL) {          // "__text", the segment's first section
            const long long rs = is64 ? (long long)ex_rd(H, posSec + 0x30, 8, false) : (long long)(int)(u32)ex_rd(H, posSec + 0x2C, 4, false);
            if (!ex_set_range(H, rs, (int)(u32)ex_rd(H, posSec + 0x28, 4, false), true)) return false;
            break;
          }
        }
      }
      pos += szCmd;
    }
    if (H.cs > count) H.cs = count;
    if (H.ce > count) H.ce = count;
    return !H.past;
  }
  return false;
}

__host__ __device__ __forceinline__ bool ex_bad_range(int cs, int ce, int count) { return cs < 0 || cs > count || ce < cs || ce > count; }   // :674, :694
__host__ __device__ __forceinline__ int ex_arch_mode(int arch) {                          // :678-691
  if (arch == 0x03 || arch == 0x3E || arch == 0x014C || arch == 0x8664 || arch == 0x1000007) return EX_X86F;
  if (arch == 0xB7 || arch == 0xAA64 || arch == 0x100000C) return EX_ARMF;
  return EX_NONE;
}
__device__ __forceinline__ void ex_take(const ExScratch& S, int b, int mode, int cs, int ce, int n) {
  const int hi = (mode == EX_ARMF) ? cs + ((ce - cs) & ~3) : ce;
  S.info[b] = make_int4(mode, cs, hi, n);
  S.exitPos[b] = hi;
  S.cstart[b] = cs;
}

// forward: size and data-type rules, parseHeader.  inverse: the header checks.  One lane per block.
__global__ void k_exe_setup(const u8* __restrict__ src, int64_t stride, const int32_t* __restrict__ d_len, int32_t* __restrict__ d_len2,
                            int32_t* __restrict__ d_flag, const int32_t* __restrict__ d_dtype, ExScratch S, int B, int inverse, int dstCap) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = d_len[b];
  const u8* s = src + (int64_t)b * stride;
  S.matches[b] = 0; S.fail[b] = 0; S.jumps[2 * b] = 0; S.jumps[2 * b + 1] = 0;
  S.info[b] = make_int4(EX_NONE, 0, 0, n);
  d_len2[b] = inverse ? 0 : n;
  d_flag[b] = (n == 0) ? 1 : 0;                                                  // :111, :375
  if (n == 0) return;
  if (inverse) {
    if (n < 9) return;                                                           // :390
    const int mode = s[0];
    if (mode != EX_MODE_X86 && mode != EX_MODE_ARM64) return;
    const int cs = (int)((u32)s[1] | ((u32)s[2] << 8) | ((u32)s[3] << 16) | ((u32)s[4] << 24));
    const int ce = (int)((u32)s[5] | ((u32)s[6] << 8) | ((u32)s[7] << 16) | ((u32)s[8] << 24));
    if (cs < 0 || ce < 9 || ce > n || cs > ce - 9 || cs > dstCap) return;        // :413-415
    S.info[b] = make_int4(mode == EX_MODE_X86 ? EX_X86I : EX_ARMI, 9 + cs, ce, n);
    return;
  }
  if (n < EX_MIN_BLOCK || n > EX_MAX_BLOCK) return;                              // :119
  const int dt = d_dtype[b];
  if (dt != DT_UNDEFINED && dt != DT_EXE && dt != DT_BIN) return;                // :130-137
  ExHdr H; H.cs = 0; H.ce = n; H.arch = 0; H.s = s; H.count = n; H.past = false;
  if (ex_parse_header(H)) {
    if (ex_bad_range(H.cs, H.ce, n)) return;
    const int m = ex_arch_mode(H.arch);
    if (m != EX_NONE) { ex_take(S, b, m, H.cs, H.ce, n); return; }
  }
  if (ex_bad_range(H.cs, H.ce, n)) return;
  S.info[b] = make_int4(EX_DET, H.cs, H.ce, n);                                  // the heuristic decides; the range stays as the header left it
}

__global__ __launch_bounds__(KZ_WG) void k_exe_map(const u8* __restrict__ src, int64_t stride, ExScratch S, int detect) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int4 I = S.info[b];
  if (detect ? (I.x != EX_DET) : (I.x < EX_X86F)) return;
  const int n = I.w, pos = t * EX_TILE + (int)threadIdx.x * EX_PER;
  if (t * EX_TILE >= n) return;
  __shared__ u32 ldsm[KZ_WG / 64];
  u64 q[3];
  ex_load(src + (int64_t)b * stride, pos, n, q);
  u32 tot;
  (void)ex_wg_excl_map(ex_thread_map(I.x, q, pos, I.y, I.z, n), ldsm, &tot);
  if (threadIdx.x == 0) S.tMap[(int64_t)b * S.T + t] = tot;
}

// one wave per block: the state at every tile's start (a block starts at an instruction start / a visited byte: state 0)
__global__ __launch_bounds__(64) void k_exe_scan(ExScratch S, int detect) {
  const int b = blockIdx.x;
  const int4 I = S.info[b];
  if (detect ? (I.x != EX_DET) : (I.x < EX_X86F)) return;
  const int tiles = (I.w + EX_TILE - 1) / EX_TILE, lane = kz_lane();
  const int64_t o = (int64_t)b * S.T;
  u32 carry = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + lane;
    u32 inc = (t < tiles) ? S.tMap[o + t] : EX_IDENT;
    for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if (lane >= d) inc = ex_compose(up, inc); }
    u32 ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = EX_IDENT;
    if (t < tiles) S.tState[o + t] = ex_nib(ex, carry);
    carry = ex_nib((u32)__shfl((int)inc, 63, 64), carry);
  }
}

// the state at the thread's first byte
#define EX_ENTER()                                                                                       \
  const int b = blockIdx.y, t = blockIdx.x;                                                              \
  const int n = I.w, mode = I.x, lo = I.y, hi = I.z, pos = t * EX_TILE + (int)threadIdx.x * EX_PER;      \
  if (t * EX_TILE >= n) return;                                                                          \
  __shared__ u32 ldsm[KZ_WG / 64];                                                                       \
  u64 q[3];                                                                                              \
  ex_load(src + (int64_t)b * stride, pos, n, q);                                                         \
  u32 tot_;                                                                                              \
  const u32 exm = ex_wg_excl_map(ex_thread_map(mode, q, pos, lo, hi, n), ldsm, &tot_);                   \
  u32 st = ex_nib(exm, S.tState[(int64_t)b * S.T + t]);

// the heuristic's counts (:701-747): the histogram of the visited bytes, x86 and ARM64 jumps
__global__ __launch_bounds__(KZ_WG) void k_exe_hist(const u8* __restrict__ src, int64_t stride, ExScratch S) {
  const int4 I = S.info[blockIdx.y];
  if (I.x != EX_DET) return;
  EX_ENTER()
  (void)lo; (void)hi;
  __shared__ u32 h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  u32 jx = 0, ja = 0;
#pragma unroll
  for (int k = 0; k < EX_PER; k++) {
    const int p = pos + k;
    if (p >= n) continue;
    const u64 win = ex_win(q, k);
    const u32 b0 = (u32)win & 0xFFu, b1 = (u32)(win >> 8) & 0xFFu, b2 = (u32)(win >> 16) & 0xFFu, b4 = (u32)(win >> 32) & 0xFFu;
    bool armTest;
    if (st == 0u) {
      atomicAdd(&h[b0], 1u);
      armTest = true;
      if (p + 4 < n && (b0 & 0xFEu) == 0xE8u) { if (b4 == 0u || b4 == 0xFFu) jx++; }            // :710-719
      else if (b0 == 0x0Fu && p + 1 < n) {                                                      // :720-734: i moves to j
        st = ((b1 == 0x38u || b1 == 0x3Au) && p + 2 < n) ? 2u : 1u;
        if ((((st == 2u) ? b2 : b1) & 0xF0u) == 0x80u) jx++;
        armTest = false;
      }
    } else { st--; armTest = (st == 0u); }                                                      // :737 uses the moved i: the last skipped byte
    if (armTest && (p & 3) == 0 && p + 4 <= n) {
      const u32 instr = (u32)win, op1 = instr & EX_ARM_OPMASK, op2 = instr & 0x7F000000u;
      if (op1 == EX_ARM_B || op1 == EX_ARM_BL || op2 == 0x34000000u || op2 == 0x3500000u) ja++;   // CBNZ as the reference writes it (:58): never equal
    }
  }
  jx = kz_wave_sum(jx); ja = kz_wave_sum(ja);
  if (kz_lane() == 0) { if (jx) atomicAdd(&S.jumps[2 * b], (int)jx); if (ja) atomicAdd(&S.jumps[2 * b + 1], (int)ja); }
  __syncthreads();
  const u32 v = h[threadIdx.x];
  if (v) atomicAdd(&S.hist[(int64_t)b * 256 + threadIdx.x], v);
}

// detectSimpleType and the thresholds (:749-771)
__global__ __launch_bounds__(256) void k_exe_decide(ExScratch S) {
  const int b = blockIdx.x;
  const int4 I = S.info[b];
  if (I.x != EX_DET) return;
  __shared__ long long lds4[4];
  const int n = I.w, tid = (int)threadIdx.x;
  const int f = (int)S.hist[(int64_t)b * 256 + tid], fEq = (int)S.hist[(int64_t)b * 256 + '='];
  const int dt = kz_detect_simple_type_wg(n, f, fEq, lds4);
  const long long small = kz_wg256_sum64(tid < 16 ? f : 0, lds4);
  if (tid != 0) return;
  const int h0 = (int)S.hist[(int64_t)b * 256], h255 = (int)S.hist[(int64_t)b * 256 + 255];
  int mode = EX_NONE;
  if (dt == DT_BIN && !(h0 < n / 10 || small > n / 2 || h255 < n / 100)) {       // :760
    if (S.jumps[2 * b] >= n / 200) mode = EX_X86F;                               // :764: x86 first
    else if (S.jumps[2 * b + 1] >= n / 200) mode = EX_ARMF;
  }
  if (mode == EX_NONE) S.info[b] = make_int4(EX_NONE, 0, 0, n);
  else ex_take(S, b, mode, I.y, I.z, n);
}

__global__ __launch_bounds__(KZ_WG) void k_exe_size(const u8* __restrict__ src, int64_t stride, ExScratch S) {
  const int4 I = S.info[blockIdx.y];
  if (I.x < EX_X86F) return;
  EX_ENTER()
  __shared__ u32 lds[32];
  const u32 st0 = st;
  u32 sum = 0, matches = 0, fail = 0;
  int exitAt = 0x7FFFFFFF;
#pragma unroll
  for (int k = 0; k < EX_PER; k++) {
    const ExStep r = ex_step(mode, st, pos + k, ex_win(q, k), lo, hi, n);
    sum += r.sz;
    matches += (r.flags & EXF_MATCH) ? 1u : 0u;
    fail |= r.flags & EXF_FAIL;
    if (r.flags & EXF_EXIT) exitAt = min(exitAt, pos + k);
    st = r.next;
  }
  S.strip[((int64_t)b * S.T + t) * KZ_WG + threadIdx.x] = (uint16_t)(st0 | (sum << 4));
  u32 total;
  (void)kz_wg_excl_sum(sum, lds, &total);
  if (threadIdx.x == 0) S.tSum[(int64_t)b * S.T + t] = total;
  matches = kz_wave_sum(matches);
  if (kz_lane() == 0 && matches) atomicAdd(&S.matches[b], (int)matches);
  if (fail) atomicOr(&S.fail[b], 1);
  if (exitAt != 0x7FFFFFFF) atomicMin(&S.exitPos[b], exitAt);
}

// offsets per tile, the block's verdict, and the forward's header (:246-260, :345-359; inverse: :487, :636 and the per-store checks)
__global__ __launch_bounds__(64) void k_exe_verdict(u8* __restrict__ dst, int64_t stride, int32_t* __restrict__ d_len2, int32_t* __restrict__ d_flag,
                                                    int32_t* __restrict__ d_dtype, ExScratch S, int dstCap) {
  const int b = blockIdx.x;
  const int4 I = S.info[b];
  if (I.x < EX_X86F) return;
  const int n = I.w, tiles = (n + EX_TILE - 1) / EX_TILE, lane = kz_lane();
  const int64_t o = (int64_t)b * S.T;
  u64 carry = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int t = base + lane;
    const u32 v = (t < tiles) ? S.tSum[o + t] : 0u;
    u64 inc = v;
    for (int d = 1; d < 64; d <<= 1) { const u64 up = __shfl_up(inc, d, 64); if (lane >= d) inc += up; }
    if (t < tiles) S.tOff[o + t] = (u32)(carry + inc - v);
    carry += __shfl(inc, 63, 64);
  }
  if (lane != 0) return;
  const bool forward = I.x <= EX_ARMF;
  bool ok;
  long long total = (long long)carry;
  if (forward) {
    total += 9;
    ok = S.matches[b] >= 16 && total <= (long long)n + n / 50;
  } else ok = !S.fail[b] && total <= (long long)dstCap;
  if (!ok) { S.info[b] = make_int4(EX_NONE, 0, 0, n); return; }                  // (k_exe_setup wrote the declined / failed result)
  d_len2[b] = (int32_t)total;
  d_flag[b] = 1;
  if (!forward) return;
  d_dtype[b] = DT_EXE;                                                           // :156-157
  u8* d = dst + (int64_t)b * stride;
  const u32 cs = (u32)S.cstart[b], at = (u32)(total - (n - S.exitPos[b]));       // dstIdx at the loop's exit: it counts the header
  d[0] = (I.x == EX_X86F) ? EX_MODE_X86 : EX_MODE_ARM64;
  for (int i = 0; i < 4; i++) { d[1 + i] = (u8)(cs >> (8 * i)); d[5 + i] = (u8)(at >> (8 * i)); }
}

__host__ __device__ __forceinline__ void ex_put32(u8* d, u32 v, bool big) {
  for (int i = 0; i < 4; i++) d[i] = (u8)(v >> (big ? 24 - 8 * i : 8 * i));
}

// the bytes of one instruction or word (r.sz >= 2) at w; o: the output offset BEHIND them
__host__ __device__ __forceinline__ void ex_emit(int mode, const ExStep& r, int p, u64 win, u32 o, u8* w) {
  const u32 b0 = (u32)win & 0xFFu;
  if (mode == EX_X86F) {
    if (r.sz == 2) { w[0] = 0x9B; w[1] = (u8)b0; return; }                     // a doubled 9B, or an escaped opcode byte
    const int32_t off = (int32_t)(u32)(win >> 8);
    const int32_t addr = p + ((((u32)(win >> 32) & 0xFFu) == 0u) ? off : -(int32_t)((0u - (u32)off) & 0xFFFFFFu));     // :236
    w[0] = (u8)b0;
    ex_put32(w + 1, (u32)addr ^ EX_MASK_ADDRESS, true);
  } else if (mode == EX_X86I) {
    const u32 be = (u32)(win >> 8);
    const int32_t addr = (int32_t)(__builtin_bswap32(be) ^ EX_MASK_ADDRESS);   // :478
    const long long off = (long long)addr - (long long)(o - 5u);               // against the opcode byte's place in the output
    const int32_t enc = (off >= 0) ? (int32_t)off : -(int32_t)((-off) & 0xFFFFFFLL);
    w[0] = (u8)b0;
    ex_put32(w + 1, (u32)enc, false);
  } else if (mode == EX_ARMF) {
    const u32 instr = (u32)win, op1 = instr & EX_ARM_OPMASK;
    u32 val = instr;
    if (r.flags) {
      int addr = p + 4 * (((int32_t)(instr << 6)) >> 6);
      if (addr < 0) addr = 0;
      val = op1 | (u32)(addr >> 2);                                            // :312
    }
    ex_put32(w, val, false);
    if (r.flags & EXF_ESC) ex_put32(w + 4, instr, false);                      // :326-335
  } else {
    const u32 instr = (u32)win, op1 = instr & EX_ARM_OPMASK;
    u32 val = instr;
    if (r.flags & EXF_ESC) val = (u32)(win >> 32);
    else if (r.flags & EXF_MATCH) {
      const int32_t addr = (int32_t)((instr & EX_ARM_ADDRMASK) << 2);
      val = op1 | ((u32)((addr - (int32_t)(o - 4u)) >> 2) & EX_ARM_ADDRMASK);  // :609-611: an arithmetic shift
    }
    ex_put32(w, val, false);
  }
}

__global__ __launch_bounds__(KZ_WG) void k_exe_emit(const u8* __restrict__ src, u8* __restrict__ dst, int64_t stride, ExScratch S) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int4 I = S.info[b];
  if (I.x < EX_X86F) return;                                                     // declined or failed: dst is left alone
  const int n = I.w, mode = I.x, lo = I.y, hi = I.z, pos = t * EX_TILE + (int)threadIdx.x * EX_PER;
  if (t * EX_TILE >= n) return;
  __shared__ u32 lds[32];
  u64 q[3];
  ex_load(src + (int64_t)b * stride, pos, n, q);
  const u32 packed = S.strip[((int64_t)b * S.T + t) * KZ_WG + threadIdx.x];
  u32 st = packed & 15u, total;
  u32 o = kz_wg_excl_sum(packed >> 4, lds, &total) + S.tOff[(int64_t)b * S.T + t] + ((mode <= EX_ARMF) ? 9u : 0u);
  u8* d = dst + (int64_t)b * stride;
#pragma unroll
  for (int k = 0; k < EX_PER; k++) {
    const int p = pos + k;
    const u64 win = ex_win(q, k);
    const ExStep r = ex_step(mode, st, p, win, lo, hi, n);
    st = r.next;
    if (r.sz == 0) continue;
    const u32 b0 = (u32)win & 0xFFu;
    u8* w = d + o;
    o += r.sz;
    if (r.sz == 1) { w[0] = (u8)b0; continue; }
    ex_emit(mode, r, p, win, o, w);
  }
}

// =================================================================================================
static size_t ex_tiles(int maxN) { return (size_t)(maxN + EX_TILE - 1) / EX_TILE + 1; }
size_t kz_exe_scratch(int B, int maxN, bool decode) {
  const size_t T = ex_tiles(maxN);
  return (size_t)B * (kz_align(T * 4, 256) * 4 + kz_align(T * KZ_WG * 2, 256) + (decode ? 0 : 1024) + 64) + 16 * 256 + 8192;
}

static int ex_alloc(kz_ctx* ctx, ExScratch& S, int B, int maxN, bool decode) {
  S.T = (int)ex_tiles(maxN);
  S.tMap = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tState = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tSum = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.tOff = (u32*)kz_arena_alloc(ctx, (size_t)B * S.T * 4);
  S.strip = (uint16_t*)kz_arena_alloc(ctx, (size_t)B * S.T * KZ_WG * 2);
  S.hist = decode ? nullptr : (u32*)kz_arena_alloc(ctx, (size_t)B * 256 * 4);
  S.info = (int4*)kz_arena_alloc(ctx, (size_t)B * 16);
  S.jumps = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 8);
  S.matches = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.fail = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.exitPos = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  S.cstart = (int32_t*)kz_arena_alloc(ctx, (size_t)B * 4);
  if (!S.cstart || (!decode && !S.hist) || !S.strip) { snprintf(ctx->err, sizeof(ctx->err), "exe: arena overflow"); return -KZ_ERR_DEVICE; }
  return 0;
}

int kz_stage_exe_forward(kz_ctx* ctx, kz_batch& bt) {
  const int B = bt.B;
  int maxN = 0;
  for (int b = 0; b < B; b++) if (bt.h_len[b] > maxN) maxN = bt.h_len[b];
  ExScratch S;
  int rc = ex_alloc(ctx, S, B, maxN, false);
  if (rc) return rc;
  const u8* src = bt.buf[bt.cur];
  u8* dst = bt.buf[bt.cur ^ 1];
  const int tiles = (maxN + EX_TILE - 1) / EX_TILE;
  KZ_HIP(hipMemsetAsync(S.hist, 0, (size_t)B * 256 * 4, ctx->stream));
  KZ_LAUNCH(ctx, KID_EXE_SETUP, k_exe_setup, dim3((B + 63) / 64), dim3(64), src, bt.stride, bt.d_len, bt.d_len2, bt.d_flag, bt.d_dtype, S, B, 0, 0);
  if (maxN >= EX_MIN_BLOCK) {
    KZ_LAUNCH(ctx, KID_EXE_MAP, k_exe_map, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S, 1);
    KZ_LAUNCH(ctx, KID_EXE_SCAN, k_exe_scan, dim3(B), dim3(64), S, 1);
    KZ_LAUNCH(ctx, KID_EXE_HIST, k_exe_hist, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S);
    KZ_LAUNCH(ctx, KID_EXE_DECIDE, k_exe_decide, dim3(B), dim3(256), S);
    KZ_LAUNCH(ctx, KID_EXE_MAP, k_exe_map, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S, 0);
    KZ_LAUNCH(ctx, KID_EXE_SCAN, k_exe_scan, dim3(B), dim3(64), S, 0);
    KZ_LAUNCH(ctx, KID_EXE_SIZE, k_exe_size, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S);
    KZ_LAUNCH(ctx, KID_EXE_VERDICT, k_exe_verdict, dim3(B), dim3(64), dst, bt.stride, bt.d_len2, bt.d_flag, bt.d_dtype, S, 0);
    KZ_LAUNCH(ctx, KID_EXE_EMIT, k_exe_emit, dim3(tiles, B), dim3(KZ_WG), src, dst, bt.stride, S);
  }
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}

int kz_stage_exe_inverse(kz_ctx* ctx, kz_batch& bt, int dstCap) {
  const int B = bt.B;
  int maxN = 0;
  for (int b = 0; b < B; b++) if (bt.h_len[b] > maxN) maxN = bt.h_len[b];
  ExScratch S;
  int rc = ex_alloc(ctx, S, B, maxN, true);
  if (rc) return rc;
  const u8* src = bt.buf[bt.cur];
  u8* dst = bt.buf[bt.cur ^ 1];
  if ((int64_t)dstCap > bt.stride) dstCap = (int)bt.stride;
  const int tiles = (maxN + EX_TILE - 1) / EX_TILE;
  KZ_LAUNCH(ctx, KID_EXE_SETUP, k_exe_setup, dim3((B + 63) / 64), dim3(64), src, bt.stride, bt.d_len, bt.d_len2, bt.d_flag, bt.d_dtype, S, B, 1, dstCap);
  if (maxN >= 9) {
    KZ_LAUNCH(ctx, KID_EXE_MAP, k_exe_map, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S, 0);
    KZ_LAUNCH(ctx, KID_EXE_SCAN, k_exe_scan, dim3(B), dim3(64), S, 0);
    KZ_LAUNCH(ctx, KID_EXE_SIZE, k_exe_size, dim3(tiles, B), dim3(KZ_WG), src, bt.stride, S);
    KZ_LAUNCH(ctx, KID_EXE_VERDICT, k_exe_verdict, dim3(B), dim3(64), dst, bt.stride, bt.d_len2, bt.d_flag, bt.d_dtype, S, dstCap);
    KZ_LAUNCH(ctx, KID_EXE_EMIT, k_exe_emit, dim3(tiles, B), dim3(KZ_WG), src, dst, bt.stride, S);
  }
  KZ_HIP(hipGetLastError());
  bt.cur ^= 1;
  { int32_t* t = bt.d_len; bt.d_len = bt.d_len2; bt.d_len2 = t; }
  return 0;
}
