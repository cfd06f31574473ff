// knz_store_check.cpp -- the host-only plan of the many-stream byte-addressed read (kanzi_amd/csrc/kz_knz_host.h: knz_read_many_args,
// knz_read_many_plan, knz_read_settle_blocks, knz_read_settle_segs) under the sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/knz_store_check.cpp -o /tmp/knz_store_check && /tmp/knz_store_check
// Every array is a heap allocation of the exact size.  The decode is stood in for by rows cut from known originals (one per stream), so
// the copy of the segments is checked byte for byte against plain slicing in a destination of exactly D[nRanges] bytes; a call over
// one stream must give knz_read_plan's plan.
#include "kz_knz_host.h"
#include <stdlib.h>
#include <memory>
#include <vector>

static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("knz_store_check FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } checked++; } while (0)
static uint32_t rnd() { static uint32_t s = 0x9E3779B9u; s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {        // a heap copy of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}
static uint8_t orig_byte(int s, int64_t i) { return (uint8_t)((i * 131) ^ (i >> 8) ^ (s * 29) ^ 0x5A); }

struct Stream { std::vector<int32_t> lens; int32_t bs; bool table, use; int32_t group; std::vector<int64_t> B; };
struct Range { int32_t s; int64_t off, len; };

static void run(std::vector<Stream>& st, const std::vector<Range>& rg, const std::vector<int>& chunkBlocks, int phase, int brokenStream = -1, int brokenBlock = -1) {
  const int32_t ns = (int32_t)st.size(), nRanges = (int32_t)rg.size();
  std::vector<std::unique_ptr<int64_t[]>> tabs;
  std::vector<KnzManyStreamIn> in;
  for (Stream& S : st) {
    S.B.assign(1, 0);
    for (int32_t l : S.lens) S.B.push_back(S.B.back() + l);
    tabs.push_back(exact(S.B));
    in.push_back(KnzManyStreamIn{S.use, S.group, (int32_t)S.lens.size(), S.bs, S.table ? tabs.back().get() : nullptr});
  }
  std::vector<int32_t> rs; std::vector<int64_t> ro, rl;
  int64_t total = 0;
  for (const Range& r : rg) { rs.push_back(r.s); ro.push_back(r.off); rl.push_back(r.len); total += r.len; }
  auto S_ = exact(rs); auto off = exact(ro); auto len = exact(rl); auto cb = exact(chunkBlocks); auto sin = exact(in);
  KnzManyReadPlan P;
  knz_read_many_plan(sin.get(), ns, S_.get(), off.get(), len.get(), nRanges, cb.get(), phase, P);
  const int64_t nr = (int64_t)P.rowStream.size(), nChunks = (int64_t)P.chunkGroup.size();
  // ---- rows: by group, stream, block, distinct; chunks: back to back, inside one group, of the group's size at the most ----
  for (int64_t r = 1; r < nr; r++) {
    const int g0 = st[(size_t)P.rowStream[(size_t)r - 1]].group, g1 = st[(size_t)P.rowStream[(size_t)r]].group;
    CHECK(g0 < g1 || (g0 == g1 && (P.rowStream[(size_t)r - 1] < P.rowStream[(size_t)r] || (P.rowStream[(size_t)r - 1] == P.rowStream[(size_t)r] && P.rowBlock[(size_t)r - 1] < P.rowBlock[(size_t)r]))), "row order");
  }
  CHECK((int64_t)P.chunkRow.size() == nChunks + 1 && P.chunkRow[0] == 0 && P.chunkRow[(size_t)nChunks] == nr, "chunk table");
  CHECK((int64_t)P.first.size() == nChunks + 1 && (int64_t)P.units.size() == nChunks && P.first[(size_t)nChunks] == (int64_t)P.segs.size(), "segment table");
  for (int64_t c = 0; c < nChunks; c++) {
    const int64_t r0 = P.chunkRow[(size_t)c], r1 = P.chunkRow[(size_t)c + 1];
    const int g = P.chunkGroup[(size_t)c];
    CHECK(r0 < r1 && r1 - r0 <= chunkBlocks[(size_t)g], "chunk size");
    for (int64_t r = r0; r < r1; r++) CHECK(st[(size_t)P.rowStream[(size_t)r]].use && st[(size_t)P.rowStream[(size_t)r]].group == g, "a row of another group");
    if (c + 1 < nChunks && P.chunkGroup[(size_t)c + 1] == g) CHECK(r1 - r0 == chunkBlocks[(size_t)g], "a chunk that is not full in front of one of its group");
    int64_t u = 0, lastDst = -1;
    std::vector<char> used((size_t)(r1 - r0), 0);
    CHECK(P.first[(size_t)c] < P.first[(size_t)c + 1], "a chunk without a segment");
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzReadSeg& s = P.segs[(size_t)i];
      CHECK(s.unit0 == u, "unit0");
      u += knz_read_units((phase + s.dst) & 15, s.len);
      CHECK(s.len > 0 && s.slot >= 0 && s.slot < r1 - r0 && s.range >= 0 && s.range < nRanges && s.dst > lastDst, "segment fields");
      lastDst = s.dst;
      const int str = P.rowStream[(size_t)(r0 + s.slot)], k = P.rowBlock[(size_t)(r0 + s.slot)];
      CHECK(str == rs[(size_t)s.range], "a segment of another stream's row");
      const int64_t blen = st[(size_t)str].table ? st[(size_t)str].B[(size_t)k + 1] - st[(size_t)str].B[(size_t)k] : st[(size_t)str].bs;
      CHECK(s.off >= 0 && (int64_t)s.off + s.len <= blen, "segment leaves its block");
      used[(size_t)s.slot] = 1;
    }
    CHECK(P.units[(size_t)c] == u, "units of a chunk");
    for (char x : used) CHECK(x, "a row no segment uses");
  }
  // ---- one stream: knz_read_plan's plan ----
  if (ns == 1 && st[0].use) {
    KnzReadPlan Q;
    knz_read_plan(sin[0].B, sin[0].nIndex, st[0].bs, off.get(), len.get(), nRanges, chunkBlocks[0], phase, Q);
    CHECK(Q.blocks == P.rowBlock && Q.first == P.first && Q.units == P.units && Q.segs.size() == P.segs.size(), "one stream: another plan");
    for (size_t i = 0; i < Q.segs.size(); i++) CHECK(memcmp(&Q.segs[i], &P.segs[i], sizeof(KnzReadSeg)) == 0, "one stream: segment %zu", i);
  }
  // ---- chunk by chunk: rows, the settle per stream, the copy ----
  std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)total]);
  if (total) memset(dst.get(), 0xA5, (size_t)total);
  std::vector<int64_t> gotv((size_t)nRanges, 0);
  auto got = exact(gotv);
  for (int64_t c = 0; c < nChunks; c++) {
    const int64_t r0 = P.chunkRow[(size_t)c], cnt = P.chunkRow[(size_t)c + 1] - r0;
    std::unique_ptr<kz_block_result[]> res(new kz_block_result[(size_t)cnt]);
    std::vector<std::unique_ptr<uint8_t[]>> rows;
    for (int64_t j = 0; j < cnt; j++) {
      const int str = P.rowStream[(size_t)(r0 + j)], k = P.rowBlock[(size_t)(r0 + j)];
      memset(&res[j], 0, sizeof(res[j]));
      res[j].length = st[(size_t)str].lens[(size_t)k];
      if (str == brokenStream && k == brokenBlock) { res[j].status = -KZ_ERR_PROCESS_BLOCK; res[j].length = 0; }
      rows.emplace_back(new uint8_t[(size_t)res[j].length]);
      for (int32_t i = 0; i < res[j].length; i++) rows.back()[i] = orig_byte(str, st[(size_t)str].B[(size_t)k] + i);
    }
    for (int64_t i = 0; i < cnt;) {
      const int str = P.rowStream[(size_t)(r0 + i)];
      int64_t j = i + 1;
      while (j < cnt && P.rowStream[(size_t)(r0 + j)] == str) j++;
      knz_read_settle_blocks(&P.rowBlock[(size_t)(r0 + i)], j - i, sin[(size_t)str].B, sin[(size_t)str].nIndex, st[(size_t)str].bs, res.get() + i);
      i = j;
    }
    knz_read_settle_segs(P.segs.data(), P.first[(size_t)c], P.first[(size_t)c + 1], res.get(), got.get());
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzReadSeg& s = P.segs[(size_t)i];
      if (s.len > 0) memcpy(dst.get() + s.dst, rows[(size_t)s.slot].get() + s.off, (size_t)s.len);   // (a read past the decoded length is reported)
    }
  }
  // ---- against plain slicing, stream by stream ----
  int64_t D = 0;
  for (int32_t r = 0; r < nRanges; r++) {
    const Stream& S = st[(size_t)rs[(size_t)r]];
    const int32_t nIndex = (int32_t)S.lens.size();
    const int64_t planEnd = S.table ? S.B[(size_t)nIndex] : (int64_t)nIndex * S.bs;
    const int64_t end = S.table ? S.B[(size_t)nIndex] : (nIndex ? (int64_t)(nIndex - 1) * S.bs + S.lens[(size_t)nIndex - 1] : 0);
    int64_t want = ro[(size_t)r] < end ? std::min<int64_t>(rl[(size_t)r], end - ro[(size_t)r]) : 0, code = 0;
    const int64_t touchedEnd = ro[(size_t)r] < planEnd ? ro[(size_t)r] + std::min<int64_t>(rl[(size_t)r], planEnd - ro[(size_t)r]) : ro[(size_t)r];
    for (int32_t k = 0; k < nIndex && !code && S.use && touchedEnd > ro[(size_t)r]; k++) {   // (a range of no bytes touches no block)
      const int64_t b0 = S.table ? S.B[(size_t)k] : (int64_t)k * S.bs, b1 = S.table ? S.B[(size_t)k + 1] : b0 + S.bs;
      if (!(b0 < touchedEnd && b1 > ro[(size_t)r])) continue;
      if (rs[(size_t)r] == brokenStream && k == brokenBlock) code = -KZ_ERR_PROCESS_BLOCK;
      if (!code && !S.table && k != nIndex - 1 && S.lens[(size_t)k] != S.bs) code = -KZ_ERR_INVALID_FILE;
    }
    if (!S.use) want = 0;                                                            // a stream that is not read: nothing of it is delivered
    if (code) CHECK(got[r] == code, "range %d: got %lld, want the code %lld", r, (long long)got[r], (long long)code);
    else {
      CHECK(got[r] == want, "range %d: got %lld, want %lld", r, (long long)got[r], (long long)want);
      for (int64_t i = 0; i < want; i++) {
        const int64_t src = ro[(size_t)r] + i;
        if (dst[(size_t)(D + i)] != orig_byte(rs[(size_t)r], S.table ? src : S.B[(size_t)(src / S.bs)] + src % S.bs)) CHECK(false, "range %d: byte %lld", r, (long long)i);
      }
      for (int64_t i = want; i < rl[(size_t)r]; i++) if (dst[(size_t)(D + i)] != 0xA5) CHECK(false, "range %d: the tail of a cut slot was written", r);
    }
    D += rl[(size_t)r];
  }
}

static void check_random() {
  for (int it = 0; it < 600; it++) {
    const int ns = 1 + (int)(rnd() % (it % 5 == 0 ? 1 : 9));
    const int ng = 1 + (int)(rnd() % 3);
    std::vector<Stream> st;
    std::vector<int> chunkBlocks;
    std::vector<int32_t> gbs;
    for (int g = 0; g < ng; g++) { chunkBlocks.push_back(1 + (int)(rnd() % 5)); gbs.push_back(1024 << (rnd() % 2)); }
    std::vector<int> seen;                                         // groups are numbered in order of first appearance
    for (int s = 0; s < ns; s++) {
      Stream S;
      int g = (int)(rnd() % ng);
      size_t at = 0;
      for (; at < seen.size(); at++) if (seen[at] == g) break;
      S.use = rnd() % 7 != 0;
      if (S.use && at == seen.size()) seen.push_back(g);
      S.group = S.use ? (int32_t)at : -1;
      S.bs = gbs[(size_t)g];
      S.table = rnd() & 1;
      const int nb = (int)(rnd() % 9);
      for (int k = 0; k < nb; k++) S.lens.push_back(S.table && (rnd() % 3 == 0) ? 1 + (int32_t)(rnd() % (uint32_t)S.bs) : S.bs);
      if (!S.table && nb) S.lens.back() = 1 + (int32_t)(rnd() % (uint32_t)S.bs);
      st.push_back(S);
    }
    std::vector<int> cbBySeen;
    for (int g : seen) cbBySeen.push_back(chunkBlocks[(size_t)g]);
    if (cbBySeen.empty()) cbBySeen.push_back(1);
    std::vector<Range> rg;
    const int nr = (int)(rnd() % 150);
    for (int i = 0; i < nr; i++) {
      const int s = (int)(rnd() % (uint32_t)ns);
      int64_t n = 0;
      for (int32_t l : st[(size_t)s].lens) n += l;
      const int kind = (int)(rnd() % 8);
      int64_t o = (int64_t)(rnd() % (uint32_t)(n + 64)), l = (int64_t)(rnd() % 100);
      if (kind == 0) l = (int64_t)(rnd() % (uint32_t)(3 * st[(size_t)s].bs));
      if (kind == 1) o = INT64_MAX - (int64_t)(rnd() % 64);
      if (kind == 2) l = 0;
      rg.push_back({s, o, l});
    }
    int bs_ = -1, bb = -1;
    if (it % 3 == 0) { bs_ = (int)(rnd() % (uint32_t)ns); if (!st[(size_t)bs_].lens.empty()) bb = (int)(rnd() % (uint32_t)st[(size_t)bs_].lens.size()); }
    run(st, rg, cbBySeen, (int)(rnd() % 16), bs_, bb);
  }
}

static void check_refusals() {
  uint8_t byte = 0;
  int64_t zero[1] = {0}, first[3] = {0, 1, 2}, down[3] = {0, 2, 1}, neg[1] = {-1}, got[1] = {0}, tf[2] = {-1, 0}, tfBad[2] = {-2, 0}, so[2] = {0, 0}, sl[2] = {1, 1}, e[2] = {0, 0};
  int32_t s0[1] = {0}, s2[1] = {2}, sn[1] = {-1};
  auto call = [&](const void* src, const int64_t* o, const int64_t* l, int32_t ns, const int64_t* f, const int64_t* bo, const int64_t* bb, const int64_t* t, const int64_t* tab,
                  const int32_t* rs, const int64_t* ro, const int64_t* rl, int32_t nr, const void* d, int64_t cap, const int64_t* g) {
    return knz_read_many_args(src, o, l, ns, f, bo, bb, t, tab, rs, ro, rl, nr, d, cap, g);
  };
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == 0, "good arguments");
  CHECK(call(&byte, so, sl, 2, first, e, e, tf, e, s0, zero, zero, 1, &byte, 0, got) == 0, "good arguments with a table");
  CHECK(call(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == 0, "an empty call");
  CHECK(call(nullptr, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null src");
  CHECK(call(&byte, nullptr, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null srcOff");
  CHECK(call(&byte, so, nullptr, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null srcLen");
  CHECK(call(&byte, so, sl, 2, nullptr, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null indexFirst");
  CHECK(call(&byte, so, sl, 2, first, nullptr, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null blockBitOff");
  CHECK(call(&byte, so, sl, 2, first, e, nullptr, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null blockBits");
  CHECK(call(&byte, so, sl, 2, first, e, e, tf, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "a table without blockByteOff");
  CHECK(call(&byte, so, sl, 2, first, e, e, tfBad, e, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "tableFirst below -1");
  CHECK(call(&byte, so, sl, 2, down, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "indexFirst descends");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s2, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "rangeStream == nStreams");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, sn, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "rangeStream < 0");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, neg, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "negative rangeOff");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, neg, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "negative rangeLen");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, nullptr, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "null rangeStream");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, nullptr, 0, got) == -KZ_ERR_INVALID_PARAM, "null dst");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, nullptr) == -KZ_ERR_INVALID_PARAM, "null got");
  CHECK(call(&byte, so, sl, -1, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "negative nStreams");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, -1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "negative nRanges");
  CHECK(call(&byte, so, sl, 2, first, e, e, nullptr, nullptr, s0, zero, zero, 1, &byte, -1, got) == -KZ_ERR_INVALID_PARAM, "negative dstCap");
  CHECK(call(&byte, so, sl, 0, nullptr, nullptr, nullptr, nullptr, nullptr, s0, zero, zero, 1, &byte, 0, got) == -KZ_ERR_INVALID_PARAM, "a range of no stream");
}

int main() {
  check_refusals();
  check_random();
  printf("knz_store_check ok: %ld checks\n", checked);
  return 0;
}
