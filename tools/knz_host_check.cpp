// knz_host_check.cpp -- the host-only core of the .knz container (kanzi_amd/csrc/kz_knz_host.h: bit I/O, stream header, prefix chain,
// block-header precheck, index-entry check, the splice plan and its host copy) under the sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/knz_host_check.cpp -o /tmp/knz_host_check && /tmp/knz_host_check
// Every buffer is a heap allocation of the exact size, so a read or write one byte outside it is reported.
#include "kz_knz_host.h"
#include <stdlib.h>
#include <memory>
#include <vector>

typedef std::unique_ptr<uint8_t[]> Buf;
static Buf buf(size_t n, int fill = 0xA5) { Buf b(new uint8_t[n]); if (n) memset(b.get(), fill, n); return b; }
static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("knz_host_check FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } checked++; } while (0)
static uint32_t rnd() { static uint32_t s = 0x2545F491u; s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

// ---- prefix width: the smallest lw >= 3 with W < 2^lw, and a prefix written by write_block read back by knz_read_prefix ----
static void check_prefix_width() {
  std::vector<uint64_t> Ws = {1, 7, 8, 15, 16};
  for (int k = 4; k <= 33; k++) { Ws.push_back((1ULL << k) - 1); Ws.push_back(1ULL << k); Ws.push_back((1ULL << k) + 1); }
  for (uint64_t W : Ws) {
    int want = 3;
    while (W >= (1ULL << want)) want++;
    const int lw = knz_prefix_width(W);
    CHECK(lw == want, "prefix width of %llu: %d, want %d", (unsigned long long)W, lw, want);
    // the prefix alone: the destination ends with it and the payload buffer is empty, so write_block must stop at the payload
    // (overflow) without reading a byte of it
    const size_t pb = (size_t)(5 + lw + 7) / 8;
    Buf d = buf(pb), none = buf(0);
    HostBits bs{d.get(), (int64_t)pb, 0, false};
    write_block(bs, none.get(), W);
    CHECK(bs.overflow && bs.pos == (uint64_t)(5 + lw), "write_block of %llu bits into a prefix-sized buffer: pos %llu", (unsigned long long)W, (unsigned long long)bs.pos);
    HostBitsIn in{d.get(), (uint64_t)(5 + lw), 0, false};
    uint64_t rd = 0;
    CHECK(knz_read_prefix(in, rd) == 0 && rd == W && in.pos == (uint64_t)(5 + lw) && !in.error, "prefix of %llu read back as %llu", (unsigned long long)W, (unsigned long long)rd);
  }
  // the end marker reads as the end, a cut prefix as a fault
  Buf e = buf(1);
  HostBits bs{e.get(), 1, 0, false};
  write_end_marker(bs);
  HostBitsIn in{e.get(), 8, 0, false};
  uint64_t rd = 1;
  CHECK(knz_read_prefix(in, rd) == KNZ_PREFIX_END && rd == 0, "end marker");
  HostBitsIn cut{e.get(), 7, 0, false};
  CHECK(knz_read_prefix(cut, rd) == -KZ_ERR_READ_FILE, "cut prefix");
}

// ---- bit I/O: putBytes / getBytes against put(., 1) / get(1), at every start phase ----
static void check_bit_io() {
  std::vector<int> lens;
  for (int l = 0; l <= 40; l++) lens.push_back(l);
  for (int l : {63, 64, 65, 127, 128, 129}) lens.push_back(l);
  for (int phase = 0; phase < 8; phase++)
    for (int L : lens) {
      const size_t sb = (size_t)(L + 7) / 8, total = (size_t)(phase + L + 7) / 8;
      Buf src = buf(sb);
      for (size_t i = 0; i < sb; i++) src[i] = (uint8_t)rnd();
      auto bit = [&](int i) { return (src[i >> 3] >> (7 - (i & 7))) & 1; };
      // cap exactly reached
      Buf a = buf(total, 0xFF), b = buf(total, 0xFF);
      HostBits wa{a.get(), (int64_t)total, 0, false}, wb{b.get(), (int64_t)total, 0, false};
      for (int i = 0; i < phase; i++) { wa.put((uint64_t)(i & 1), 1); wb.put((uint64_t)(i & 1), 1); }
      wa.putBytes(src.get(), (uint64_t)L);
      for (int i = 0; i < L; i++) wb.put((uint64_t)bit(i), 1);
      CHECK(!wa.overflow && !wb.overflow && wa.pos == wb.pos && wa.pos == (uint64_t)(phase + L), "putBytes phase %d len %d: pos %llu", phase, L, (unsigned long long)wa.pos);
      CHECK(total == 0 || memcmp(a.get(), b.get(), total) == 0, "putBytes phase %d len %d differs from bit-by-bit put", phase, L);
      // read back, both ways
      HostBitsIn ra{a.get(), (uint64_t)(phase + L), 0, false}, rb{a.get(), (uint64_t)(phase + L), 0, false};
      for (int i = 0; i < phase; i++) { CHECK(ra.get(1) == (uint64_t)(i & 1), "phase bit %d", i); rb.get(1); }
      Buf out = buf(sb, 0xFF);
      ra.getBytes(out.get(), (uint64_t)L);
      CHECK(!ra.error && ra.pos == (uint64_t)(phase + L), "getBytes phase %d len %d", phase, L);
      for (int i = 0; i < L; i++) {
        const int g = (int)rb.get(1);
        CHECK(g == bit(i) && ((out[i >> 3] >> (7 - (i & 7))) & 1) == bit(i), "bit %d of phase %d len %d", i, phase, L);
      }
      CHECK(!rb.error, "get(1) phase %d len %d", phase, L);
      if (L & 7) CHECK((out[sb - 1] & (0xFF >> (L & 7))) == 0, "getBytes phase %d len %d: spare bits not zero", phase, L);
      // one bit more than there is: an error, nothing read outside
      CHECK(rb.get(1) == 0 && rb.error, "get past the end, phase %d len %d", phase, L);
      if (L > 0) {
        HostBitsIn rs{a.get(), (uint64_t)(phase + L - 1), (uint64_t)phase, false};
        Buf o2 = buf(sb, 0xFF);
        rs.getBytes(o2.get(), (uint64_t)L);
        CHECK(rs.error, "getBytes past the end, phase %d len %d", phase, L);
      }
      // cap one byte short: overflow, nothing written
      if (L > 0 && total >= 1 && total - 1 >= (size_t)(phase + 7) / 8) {
        const size_t cap = total - 1;
        Buf c = buf(cap, 0xFF), ref = buf(cap, 0xFF);
        HostBits wc{c.get(), (int64_t)cap, 0, false}, wr{ref.get(), (int64_t)cap, 0, false};
        for (int i = 0; i < phase; i++) { wc.put((uint64_t)(i & 1), 1); wr.put((uint64_t)(i & 1), 1); }
        wc.putBytes(src.get(), (uint64_t)L);
        CHECK(wc.overflow && wc.pos == (uint64_t)phase && (cap == 0 || memcmp(c.get(), ref.get(), cap) == 0), "putBytes into a short buffer, phase %d len %d", phase, L);
        wr.put(0, L > 64 ? 64 : L);
        if (L <= 64) CHECK(wr.overflow && wr.pos == (uint64_t)phase && (cap == 0 || memcmp(c.get(), ref.get(), cap) == 0), "put into a short buffer, phase %d len %d", phase, L);
      }
    }
}

// ---- stream header: round trip, and every truncation an error ----
static void check_stream_header() {
  const int64_t ns[] = {0, 1, 65535, 65536, 1LL << 30, (1LL << 30) + 1, (1LL << 32) - 1, 1LL << 32, (1LL << 48) - 1, 1LL << 48};
  const uint64_t tt = (2ULL << 42) | (3ULL << 36);
  for (int64_t n : ns)
    for (int chk = 0; chk <= 2; chk++)
      for (int32_t bsz : {1024, 1 << 30}) {
        Buf probe = buf(32);
        HostBits p{probe.get(), 32, 0, false};
        const int szMask = write_stream_header(p, tt, 1, bsz, n, chk);
        CHECK(!p.overflow && (p.pos & 7) == 0 && p.pos == (uint64_t)(160 + 16 * szMask), "header of n %lld: %llu bits", (long long)n, (unsigned long long)p.pos);
        const size_t len = (size_t)(p.pos >> 3);
        Buf h = buf(len);
        HostBits w{h.get(), (int64_t)len, 0, false};
        write_stream_header(w, tt, 1, bsz, n, chk);
        CHECK(!w.overflow && w.pos == p.pos, "header into its exact size");
        HostBitsIn in{h.get(), (uint64_t)len * 8, 0, false};
        KnzHeader k;
        const int rc = read_stream_header(in, k, nullptr, 0);
        const int64_t wantSize = (n != 0 && n < (1LL << 48)) ? n : 0;
        CHECK(rc == 0 && in.pos == p.pos && k.chkKind == chk && k.entropyType == 1 && k.transformType == tt && k.blockSize == bsz && k.szMask == szMask && k.inputSize == wantSize,
              "header round trip n %lld chk %d bs %d: rc %d size %lld", (long long)n, chk, bsz, rc, (long long)k.inputSize);
        for (size_t t = 0; t < len; t++) {
          Buf cut = buf(t);
          if (t) memcpy(cut.get(), h.get(), t);
          HostBitsIn ci{cut.get(), (uint64_t)t * 8, 0, false};
          KnzHeader kc;
          CHECK(read_stream_header(ci, kc, nullptr, 0) < 0, "header of %zu bytes cut to %zu reads as whole", len, t);
        }
        // a short destination: overflow, nothing outside
        if (len > 0) { Buf s = buf(len - 1); HostBits ws{s.get(), (int64_t)len - 1, 0, false}; write_stream_header(ws, tt, 1, bsz, n, chk); CHECK(ws.overflow, "header into a short buffer"); }
      }
  char err[128] = {0};
  Buf v = buf(5, 0);
  HostBits w{v.get(), 5, 0, false};
  w.put(0x4B414E5A, 32); w.put(6, 4);
  HostBitsIn in{v.get(), 40, 0, false};
  KnzHeader k;
  CHECK(read_stream_header(in, k, err, sizeof(err)) == -KZ_ERR_STREAM_VERSION && err[0], "version 6");
}

// ---- knz_check_entry: the true entries of a stream, and their neighbours ----
static void check_entries() {
  const uint64_t Ws[] = {9, 64, 100, 1000, 7, 4096 + 3};
  const int nb = (int)(sizeof(Ws) / sizeof(Ws[0]));
  const size_t cap = 4096;
  Buf tmp = buf(cap);
  HostBits w{tmp.get(), (int64_t)cap, 0, false};
  write_stream_header(w, 2ULL << 42, 0, 65536, 12345, 0);
  const int64_t hdrEnd = (int64_t)w.pos;
  int64_t off[8];
  for (int i = 0; i < nb; i++) {
    const size_t pb = (size_t)(Ws[i] + 7) / 8;
    Buf pay = buf(pb);
    for (size_t j = 0; j < pb; j++) pay[j] = (uint8_t)rnd();
    off[i] = (int64_t)w.pos + 5 + knz_prefix_width(Ws[i]);
    write_block(w, pay.get(), Ws[i]);
    CHECK((int64_t)w.pos == off[i] + (int64_t)Ws[i], "write_block %d", i);
  }
  write_end_marker(w);
  CHECK(!w.overflow, "stream of the entry check");
  const int64_t n = (int64_t)((w.pos + 7) >> 3), nbits = n * 8;
  Buf s = buf((size_t)n);
  memcpy(s.get(), tmp.get(), (size_t)n);
  // the chain of prefixes gives the same entries
  HostBitsIn in{s.get(), (uint64_t)nbits, (uint64_t)hdrEnd, false};
  for (int i = 0; i < nb; i++) {
    uint64_t rd = 0;
    CHECK(knz_read_prefix(in, rd) == 0 && rd == Ws[i] && (int64_t)in.pos == off[i], "prefix %d on the chain", i);
    in.pos += rd;
  }
  uint64_t rd = 1;
  CHECK(knz_read_prefix(in, rd) == KNZ_PREFIX_END, "end of the chain");
  for (int i = 0; i < nb; i++) {
    const int64_t o = off[i], W = (int64_t)Ws[i];
    CHECK(knz_check_entry(s.get(), n, hdrEnd, o, W), "true entry %d refused", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o - 1, W), "entry %d at off - 1", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o + 1, W), "entry %d at off + 1", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o, W - 1), "entry %d with W - 1", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o, W + 1), "entry %d with W + 1", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, hdrEnd, W), "entry %d at hdrEnd", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, nbits, W), "entry %d at nbits", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o, 0), "entry %d with W = 0", i);
    CHECK(!knz_check_entry(s.get(), n, hdrEnd, o, 1LL << 34), "entry %d with W = 2^34", i);
  }
}

// ---- precheck_block_header and knz_check_block: whole and truncated block headers ----
static void check_block_header() {
  const int blockSize = 1024;
  for (int nbFunctions : {1, 5})
    for (int hi : {0, 0x80})
      for (int sk : {0, 0x10})
        for (int dataSize = 1; dataSize <= 4; dataSize++)
          for (int chk = 0; chk <= 2; chk++) {
            const uint32_t mode = (uint32_t)(hi | sk | ((dataSize - 1) << 5) | 0x05);
            const bool hasSkip = hi ? (sk && nbFunctions > 4) : sk != 0;
            const uint32_t skipFlags = hasSkip ? 0x3Cu : ((hi && !sk) ? 0u : (((mode << 4) | 0x0F) & 0xFF));   // (0x80 alone: no transform is skipped)
            const uint32_t preLen = dataSize == 1 ? 200 : 1000;
            const int headerSize = 1 + (hasSkip ? 1 : 0) + dataSize + 1;
            const uint64_t W = (uint64_t)(preLen + headerSize + (chk == 2 ? 8 : chk == 1 ? 4 : 0)) * 8;
            const uint32_t HASH = 0x1E35A7BDu;
            uint32_t c = HASH * 0x01030507u;
            c = mix32(c, HASH, mode); c = mix32(c, HASH, skipFlags); c = mix32(c, HASH, preLen);
            c = mix32(c, HASH, (uint32_t)(W >> 32)); c = mix32(c, HASH, (uint32_t)W);
            c = (c >> 23) ^ (c >> 3);
            Buf h = buf((size_t)headerSize);
            HostBits w{h.get(), headerSize, 0, false};
            w.put(mode, 8);
            if (hasSkip) w.put(skipFlags, 8);
            w.put(preLen, 8 * dataSize);
            w.put(c & 0xFF, 8);
            CHECK(!w.overflow && w.pos == (uint64_t)headerSize * 8, "block header built");
            const HostBitsIn whole{h.get(), (uint64_t)headerSize * 8, 0, false};
            CHECK(precheck_block_header(whole, W, nbFunctions, blockSize, chk) == 0, "whole block header, mode %02x nbf %d chk %d", mode, nbFunctions, chk);
            {
              Buf bad = buf((size_t)headerSize);
              memcpy(bad.get(), h.get(), (size_t)headerSize);
              bad[headerSize - 1] ^= 1;
              const HostBitsIn bi{bad.get(), (uint64_t)headerSize * 8, 0, false};
              CHECK(precheck_block_header(bi, W, nbFunctions, blockSize, chk) == -KZ_ERR_CRC_CHECK, "block header with another checksum byte, mode %02x", mode);
            }
            CHECK(precheck_block_header(whole, W + 8, nbFunctions, blockSize, chk) < 0, "block header under a longer W, mode %02x", mode);
            CHECK(precheck_block_header(whole, 7, nbFunctions, blockSize, chk) == -KZ_ERR_BLOCK_SIZE, "W = 7");
            for (int t = 1; t <= 2 && t < headerSize; t++) {
              Buf cut = buf((size_t)t);
              memcpy(cut.get(), h.get(), (size_t)t);
              const HostBitsIn ci{cut.get(), (uint64_t)t * 8, 0, false};
              CHECK(precheck_block_header(ci, W, nbFunctions, blockSize, chk) < 0, "block header cut to %d bytes, mode %02x", t, mode);
            }
            // the three checks of a reader, in their order
            KnzPlan P;
            memset(&P, 0, sizeof(P));
            P.h.blockSize = blockSize; P.h.chkKind = chk; P.nbFunctions = nbFunctions; P.iS = knz_dec_row_stride(blockSize);
            CHECK(knz_check_block(whole, W, 1000, 1000 + W, P) == 0, "knz_check_block, block that ends with the stream");
            CHECK(knz_check_block(whole, W, 1000, 1000 + W - 1, P) == -KZ_ERR_READ_FILE, "knz_check_block, payload past the stream");
            CHECK(knz_check_block(whole, W, 1000, 1000 + W - 1, P, false) == 0, "knz_check_block without the end check");
            P.iS = (int64_t)(W >> 3) + 63;
            CHECK(knz_check_block(whole, W, 1000, 1000 + W - 1, P) == -KZ_ERR_BLOCK_SIZE, "knz_check_block, staging row bound first");
          }
}

// ---- the small rules ----
static void check_rules() {
  CHECK(knz_chk_kind(0) == 0 && knz_chk_kind(32) == 1 && knz_chk_kind(64) == 2 && knz_chk_kind(16) == -1 && knz_chk_kind(-32) == -1, "knz_chk_kind");
  for (int k = 0; k <= 2; k++) CHECK(knz_chk_kind(knz_chk_bits(k)) == k, "knz_chk_bits %d", k);
  CHECK(knz_block_size_ok(1024) && knz_block_size_ok(1 << 30) && !knz_block_size_ok(1008) && !knz_block_size_ok((1 << 30) + 16) && !knz_block_size_ok(1025) && !knz_block_size_ok(-16), "knz_block_size_ok");
  CHECK(knz_nb_functions(0) == 1 && knz_nb_functions(2ULL << 42) == 1 && knz_nb_functions((2ULL << 42) | 1) == 2 && knz_nb_functions(0x0000FFFFFFFFFFFFULL) == 8, "knz_nb_functions");
  for (int32_t b : {1024, 1040, 65536, 1 << 22, 1 << 30}) {
    const int64_t s = knz_dec_row_stride(b), need = (int64_t)b + (b >> 3) + 1024 + 64;
    CHECK(s >= need && s < need + 256 && (s & 255) == 0, "knz_dec_row_stride %d", b);
  }
  CHECK(knz_fit_blocks(0, 1024) == 0 && knz_fit_blocks(-5, 1024) == 0 && knz_fit_blocks(1, 1024) == 1 && knz_fit_blocks(1024, 1024) == 1 && knz_fit_blocks(1025, 1024) == 2, "knz_fit_blocks");
  kz_block_result r;
  memset(&r, 0, sizeof(r));
  r.length = 1024;
  CHECK(knz_block_verdict(r, 1024, 10, 1034) == 0 && knz_block_verdict(r, 1024, 11, 1034) == -KZ_ERR_WRITE_FILE, "verdict: room");
  r.length = 1025;
  CHECK(knz_block_verdict(r, 1024, 0, 10) == -KZ_ERR_PROCESS_BLOCK, "verdict: length before room");
  r.status = -KZ_ERR_CRC_CHECK;
  CHECK(knz_block_verdict(r, 1024, 0, 10) == -KZ_ERR_CRC_CHECK, "verdict: status first");
}

// ---- splice: the plan and the host copy on sources and destinations of the exact size ----
struct SpliceSrc { Buf s; int64_t n, hdrEnd; std::vector<int64_t> off, W; std::vector<Buf> pay; };
static SpliceSrc splice_stream(const std::vector<uint64_t>& Ws, uint64_t tt, int ent, int bsz, int chk) {
  SpliceSrc S;
  const size_t cap = 1 << 16;
  Buf tmp = buf(cap);
  HostBits w{tmp.get(), (int64_t)cap, 0, false};
  write_stream_header(w, tt, (uint32_t)ent, bsz, 4000, chk);
  S.hdrEnd = (int64_t)w.pos;
  for (uint64_t W : Ws) {
    const size_t pb = (size_t)(W + 7) / 8;
    Buf pay = buf(pb);
    for (size_t j = 0; j < pb; j++) pay[j] = (uint8_t)rnd();
    S.off.push_back((int64_t)w.pos + 5 + knz_prefix_width(W));
    S.W.push_back((int64_t)W);
    write_block(w, pay.get(), W);
    S.pay.push_back(std::move(pay));
  }
  write_end_marker(w);
  CHECK(!w.overflow, "splice source built");
  S.n = (int64_t)((w.pos + 7) >> 3);
  S.s = buf((size_t)S.n);
  memcpy(S.s.get(), tmp.get(), (size_t)S.n);
  return S;
}
static void check_splice() {
  const uint64_t tt = 2ULL << 42;
  SpliceSrc A = splice_stream({9, 64, 100, 1000, 7, 4096 * 8 + 3, 33}, tt, 1, 1024, 1);
  SpliceSrc B = splice_stream({801, 15, 8 * 5000}, tt, 1, 1024, 1);
  // the two sources back to back in one allocation of the exact size
  const int64_t total = A.n + B.n;
  Buf both = buf((size_t)total);
  memcpy(both.get(), A.s.get(), (size_t)A.n);
  memcpy(both.get() + A.n, B.s.get(), (size_t)B.n);
  const int64_t srcOff[2] = {0, A.n}, srcLen[2] = {A.n, B.n};
  const SpliceSrc* S[2] = {&A, &B};
  // pieces: interleaved, reversed, with repeats, the sources' last blocks among them
  std::vector<int32_t> ps; std::vector<int64_t> po, pw;
  const int order[][2] = {{1, 2}, {0, 6}, {0, 0}, {1, 0}, {0, 5}, {0, 5}, {1, 1}, {0, 3}, {0, 4}, {0, 1}, {0, 2}, {1, 2}};
  for (auto& o : order) { ps.push_back(o[0]); po.push_back(S[o[0]]->off[o[1]]); pw.push_back(S[o[0]]->W[o[1]]); }
  const int np = (int)ps.size();
  for (int64_t inputSize : {(int64_t)0, (int64_t)70000, (int64_t)1 << 33}) {
    const int64_t bound = knz_splice_bound(pw.data(), np);
    Buf want = buf((size_t)bound);
    HostBits w{want.get(), bound, 0, false};
    write_stream_header(w, tt, 1, 1024, inputSize, 1);
    for (auto& o : order) write_block(w, S[o[0]]->pay[o[1]].get(), (uint64_t)S[o[0]]->W[o[1]]);
    write_end_marker(w);
    const int64_t size = (int64_t)((w.pos + 7) >> 3);
    CHECK(!w.overflow && size <= bound, "splice bound %lld, size %lld", (long long)bound, (long long)size);
    Buf d = buf((size_t)size);                                     // dstCap exact
    const int64_t rc = knz_splice_host(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), np, inputSize, d.get(), size);
    CHECK(rc == size && memcmp(d.get(), want.get(), (size_t)size) == 0, "splice of %d pieces: rc %lld, want %lld", np, (long long)rc, (long long)size);
    Buf e = buf((size_t)size - 1), poison = buf((size_t)size - 1);  // one byte less: refused, nothing written
    CHECK(knz_splice_host(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), np, inputSize, e.get(), size - 1) == -KZ_ERR_WRITE_FILE &&
          memcmp(e.get(), poison.get(), (size_t)size - 1) == 0, "splice into a destination one byte short");
  }
  // no pieces: header and end marker
  {
    Buf d = buf(21);
    CHECK(knz_splice_host(both.get(), srcOff, srcLen, 2, nullptr, nullptr, nullptr, 0, 0, d.get(), 21) == 21 && d[20] == 0, "splice of no pieces");
    CHECK(knz_splice_host(both.get(), srcOff, srcLen, 2, nullptr, nullptr, nullptr, 0, 0, d.get(), 20) == -KZ_ERR_WRITE_FILE, "splice of no pieces, short");
  }
  // refusals: dst stays poisoned
  const int64_t cap = knz_splice_bound(pw.data(), np);
  Buf d = buf((size_t)cap), poison = buf((size_t)cap);
  auto run = [&](const uint8_t* src, const int64_t* so, const int64_t* sl, int ns, const int32_t* s, const int64_t* o, const int64_t* w_, int n, int64_t isz, uint8_t* dst, int64_t c) {
    const int64_t rc = knz_splice_host(src, so, sl, ns, s, o, w_, n, isz, dst, c);
    CHECK(memcmp(d.get(), poison.get(), (size_t)cap) == 0, "a refused splice wrote to dst (rc %lld)", (long long)rc);
    return rc;
  };
  CHECK(run(nullptr, srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "null src");
  CHECK(run(both.get(), nullptr, srcLen, 2, ps.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "null srcOff");
  CHECK(run(both.get(), srcOff, srcLen, 0, ps.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "nSrc 0");
  CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), -1, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "nPieces -1");
  CHECK(run(both.get(), srcOff, srcLen, 2, nullptr, po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "null pieceSrc");
  CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), np, -1, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "inputSize -1");
  CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), pw.data(), np, 0, nullptr, cap) == -KZ_ERR_INVALID_PARAM, "null dst");
  { const int64_t bad[2] = {0, -1}; CHECK(run(both.get(), srcOff, bad, 2, ps.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "negative srcLen"); }
  for (int32_t v : {-1, 2}) { std::vector<int32_t> b = ps; b[3] = v; CHECK(run(both.get(), srcOff, srcLen, 2, b.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "pieceSrc %d", v); }
  // a piece named with the other source, shifted, lengthened, with W out of range
  { std::vector<int32_t> b = ps; b[0] = 0; CHECK(run(both.get(), srcOff, srcLen, 2, b.data(), po.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "piece of the other source"); }
  for (int dlt : {-1, 1}) {
    std::vector<int64_t> o = po; o[np - 1] += dlt;
    CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), o.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "piece off %+d", dlt);
    std::vector<int64_t> w_ = pw; w_[np - 1] += dlt;
    CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), w_.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "piece W %+d", dlt);
  }
  for (int64_t v : {(int64_t)0, (int64_t)-5, (int64_t)1 << 34, INT64_MAX}) {
    std::vector<int64_t> w_ = pw; w_[2] = v;
    CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), po.data(), w_.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "piece W %lld", (long long)v);
    std::vector<int64_t> o = po; o[2] = v;
    CHECK(run(both.get(), srcOff, srcLen, 2, ps.data(), o.data(), pw.data(), np, 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "piece off %lld", (long long)v);
  }
  // a bad header in a source that no piece names; sources that disagree in each of the four
  {
    std::vector<int32_t> onlyA; std::vector<int64_t> oA, wA;
    for (int i = 0; i < np; i++) if (ps[i] == 0) { onlyA.push_back(0); oA.push_back(po[i]); wA.push_back(pw[i]); }
    Buf bad = buf((size_t)total);
    memcpy(bad.get(), both.get(), (size_t)total);
    bad[A.n] ^= 0x40;
    CHECK(run(bad.get(), srcOff, srcLen, 2, onlyA.data(), oA.data(), wA.data(), (int)onlyA.size(), 0, d.get(), cap) == -KZ_ERR_INVALID_FILE, "magic of an unnamed source");
    memcpy(bad.get(), both.get(), (size_t)total);
    bad[A.n + 19] ^= 1;
    CHECK(run(bad.get(), srcOff, srcLen, 2, onlyA.data(), oA.data(), wA.data(), (int)onlyA.size(), 0, d.get(), cap) == -KZ_ERR_CRC_CHECK, "header checksum of an unnamed source");
    const int64_t shortLen[2] = {A.n, 10};
    CHECK(run(both.get(), srcOff, shortLen, 2, onlyA.data(), oA.data(), wA.data(), (int)onlyA.size(), 0, d.get(), cap) < 0, "a source of 10 bytes");
    struct { uint64_t tt; int ent, bsz, chk; const char* what; } other[] = {{3ULL << 42, 1, 1024, 1, "the transform word"}, {tt, 2, 1024, 1, "the entropy id"},
                                                                           {tt, 1, 2048, 1, "the block size"}, {tt, 1, 1024, 2, "the checksum kind"}};
    for (auto& o : other) {
      SpliceSrc C = splice_stream({801, 15}, o.tt, o.ent, o.bsz, o.chk);
      Buf two = buf((size_t)(A.n + C.n));
      memcpy(two.get(), A.s.get(), (size_t)A.n);
      memcpy(two.get() + A.n, C.s.get(), (size_t)C.n);
      const int64_t so[2] = {0, A.n}, sl[2] = {A.n, C.n};
      CHECK(run(two.get(), so, sl, 2, onlyA.data(), oA.data(), wA.data(), (int)onlyA.size(), 0, d.get(), cap) == -KZ_ERR_INVALID_PARAM, "sources that differ in %s", o.what);
      KnzSplice P; int64_t he[2]; char err[128] = "";
      CHECK(knz_splice_sources(two.get(), so, sl, 2, P, he, err, sizeof(err)) == -KZ_ERR_INVALID_PARAM && strstr(err, "source 1 differs from source 0 in") && strstr(err, o.what), "text: %s", err);
    }
  }
  // a source cut inside a prefix and inside a payload, at every byte: the pieces in front of the cut are spliced, a piece that the cut
  // touches is refused, and nothing is read behind the cut (the source is a heap buffer of the cut's size)
  for (int64_t cut = A.hdrEnd / 8; cut < A.n; cut += (cut < 200 ? 1 : 97)) {
    Buf c = buf((size_t)cut);
    memcpy(c.get(), A.s.get(), (size_t)cut);
    const int64_t so[1] = {0}, sl[1] = {cut};
    for (size_t k = 0; k < A.W.size(); k++) {
      const int32_t one = 0;
      const bool whole = A.off[k] + A.W[k] <= cut * 8;
      const int64_t rc = knz_splice_host(c.get(), so, sl, 1, &one, &A.off[k], &A.W[k], 1, 0, d.get(), cap);
      if (whole) {
        CHECK(rc > 0, "piece %zu in front of a cut at %lld: %lld", k, (long long)cut, (long long)rc);
        HostBitsIn in{d.get(), (uint64_t)rc * 8, 160 + 5 + (uint64_t)knz_prefix_width((uint64_t)A.W[k]), false};
        Buf back = buf((size_t)(A.W[k] + 7) / 8);
        in.getBytes(back.get(), (uint64_t)A.W[k]);
        const size_t fullB = (size_t)A.W[k] / 8;
        CHECK(!in.error && memcmp(back.get(), A.pay[k].get(), fullB) == 0, "payload of piece %zu in front of a cut", k);
        memset(d.get(), 0xA5, (size_t)cap);
      } else CHECK(rc == -KZ_ERR_INVALID_PARAM && memcmp(d.get(), poison.get(), (size_t)cap) == 0, "piece %zu behind a cut at %lld: %lld", k, (long long)cut, (long long)rc);
    }
  }
  // the bound's own refusals
  { const int64_t w1[1] = {-1}, w2[1] = {1LL << 34}; CHECK(knz_splice_bound(w1, 1) == -KZ_ERR_INVALID_PARAM && knz_splice_bound(w2, 1) == -KZ_ERR_INVALID_PARAM && knz_splice_bound(nullptr, 1) == -KZ_ERR_INVALID_PARAM && knz_splice_bound(nullptr, 0) == 27, "splice bound refusals"); }
}

// ---- precheck_block_header over the 64-bit header word (knz_precheck_word) against the byte-by-byte reader it replaced, restated
//      here: the same code for every header, every W and every place where the stream may end inside or behind the header ----
static int precheck_by_bytes(HostBitsIn bs, uint64_t W, int nbFunctions, int blockSize, int chkKind) {
  if (W < 8) return -KZ_ERR_BLOCK_SIZE;
  const uint32_t mode = (uint32_t)bs.get(8);
  uint32_t skipFlags = 0;
  bool hasSkip = false;
  if (mode & 0x80) {
    if (mode & 0x10) { if (nbFunctions > 4) hasSkip = true; else skipFlags = ((mode << 4) | 0x0F) & 0xFF; }
  } else if (mode & 0x10) hasSkip = true;
  else skipFlags = ((mode << 4) | 0x0F) & 0xFF;
  const int dataSize = 1 + (int)((mode >> 5) & 3);
  const int headerSize = 1 + (hasSkip ? 1 : 0) + dataSize + 1;
  if (W < (uint64_t)headerSize * 8) return -KZ_ERR_BLOCK_SIZE;
  if (hasSkip) skipFlags = (uint32_t)bs.get(8);
  uint32_t preLen = 0;
  for (int i = 0; i < dataSize; i++) preLen = (preLen << 8) | (uint32_t)bs.get(8);
  const uint32_t ck = (uint32_t)bs.get(8);
  if (bs.error) return -KZ_ERR_READ_FILE;
  const uint32_t HASH = 0x1E35A7BDu;
  uint32_t c = HASH * 0x01030507u;
  c = mix32(c, HASH, mode & 0xFF);
  c = mix32(c, HASH, skipFlags & 0xFF);
  c = mix32(c, HASH, preLen);
  c = mix32(c, HASH, (uint32_t)(W >> 32));
  c = mix32(c, HASH, (uint32_t)W);
  c = (c >> 23) ^ (c >> 3);
  if (ck != (c & 0xFF)) return -KZ_ERR_CRC_CHECK;
  const int64_t maxTL = std::min<int64_t>(std::max<int64_t>((int64_t)blockSize + blockSize / 2, 2048), 1LL << 30);
  if ((int32_t)preLen < 0 || (int64_t)preLen > maxTL) return -KZ_ERR_READ_FILE;
  const int checksumSize = (chkKind == 2) ? 8 : (chkKind == 1 ? 4 : 0);
  if ((int64_t)((W + 7) >> 3) > (int64_t)preLen + headerSize + checksumSize) return -KZ_ERR_BLOCK_SIZE;
  return 0;
}
static void check_precheck_forms() {
  long codes[6] = {0, 0, 0, 0, 0, 0};
  for (int it = 0; it < 40000; it++) {
    const int phase = (int)(rnd() % 8), nbf = (it & 1) ? 3 : 6, chk = (int)(rnd() % 3);
    const int blockSize = (it % 3) ? 1024 : 65536;
    uint8_t raw[12];
    for (int i = 0; i < 12; i++) raw[i] = (uint8_t)rnd();
    if (it % 4 == 0) raw[0] = (uint8_t)(rnd() & 0x9F);                      // one length byte, so that small lengths pass the later checks
    const Buf b = buf(12);
    memcpy(b.get(), raw, 12);
    uint64_t W = (it % 5 == 0) ? rnd() % 80 : (rnd() % 3 ? 8 * (uint64_t)(rnd() % 300) : ((uint64_t)rnd() << 3) | rnd() % 8);
    if (it % 2 == 0) {                                                       // a checksum byte that fits: the checks behind it are reached
      HostBitsIn t{b.get(), 96, (uint64_t)phase, false};
      const uint32_t mode = (uint32_t)t.get(8);
      const bool hasSkip = (mode & 0x10) && (!(mode & 0x80) || nbf > 4);
      uint32_t skip = hasSkip ? (uint32_t)t.get(8) : (((mode & 0x80) && !(mode & 0x10)) ? 0u : (((mode << 4) | 0x0F) & 0xFF));
      const int ds = 1 + (int)((mode >> 5) & 3);
      uint32_t pre = 0;
      for (int i = 0; i < ds; i++) pre = (pre << 8) | (uint32_t)t.get(8);
      const uint32_t HASH = 0x1E35A7BDu;
      uint32_t c = HASH * 0x01030507u;
      c = mix32(c, HASH, mode); c = mix32(c, HASH, skip); c = mix32(c, HASH, pre); c = mix32(c, HASH, (uint32_t)(W >> 32)); c = mix32(c, HASH, (uint32_t)W);
      const uint32_t want = ((c >> 23) ^ (c >> 3)) & 0xFF;
      for (int k = 0; k < 8; k++) {                                           // at the place of the checksum byte, whatever the bit phase
        const uint64_t bit = t.pos + k;
        const uint8_t m = (uint8_t)(0x80 >> (bit & 7));
        if ((want >> (7 - k)) & 1) b.get()[bit >> 3] |= m; else b.get()[bit >> 3] &= (uint8_t)~m;
      }
    }
    for (uint64_t nbits = (uint64_t)phase; nbits <= 96; nbits++) {          // the stream ends anywhere from the block's first bit on
      const HostBitsIn at{b.get(), nbits, (uint64_t)phase, false};
      const int a = precheck_by_bytes(at, W, nbf, blockSize, chk), n = precheck_block_header(at, W, nbf, blockSize, chk);
      CHECK(a == n, "precheck forms differ: %d against %d (W %llu, phase %d, %llu bits, %d functions)", a, n, (unsigned long long)W, phase, (unsigned long long)nbits, nbf);
      codes[a == 0 ? 0 : (a == -KZ_ERR_BLOCK_SIZE ? 1 : (a == -KZ_ERR_READ_FILE ? 2 : (a == -KZ_ERR_CRC_CHECK ? 3 : 4)))]++;
    }
  }
  CHECK(codes[0] > 1000 && codes[1] > 1000 && codes[2] > 1000 && codes[3] > 1000 && codes[4] == 0, "codes reached: %ld ok, %ld size, %ld read, %ld crc, %ld other",
        codes[0], codes[1], codes[2], codes[3], codes[4]);
}

int main() {
  check_prefix_width();
  check_bit_io();
  check_stream_header();
  check_entries();
  check_block_header();
  check_precheck_forms();
  check_rules();
  check_splice();
  printf("knz_host_check ok: %ld checks\n", checked);
  return 0;
}
