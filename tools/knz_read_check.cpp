// knz_read_check.cpp -- the host-only plan of the byte-addressed reads (kanzi_amd/csrc/kz_knz_host.h: knz_read_args, knz_read_table,
// knz_read_total, knz_read_plan, knz_read_settle) under the sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/knz_read_check.cpp -o /tmp/knz_read_check && /tmp/knz_read_check
// Every array is a heap allocation of the exact size, so a read or write one element outside it is reported.  The decode is stood
// in for by rows cut from a known original, so the copy of the segments (what kz_read_bytes does with memcpy) is checked byte for
// byte against plain slicing, in a destination of exactly D[nRanges] bytes.
#include "kz_knz_host.h"
#include <stdlib.h>
#include <memory>
#include <vector>

static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("knz_read_check FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } checked++; } while (0)
static uint32_t rnd() { static uint32_t s = 0x2545F491u; s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {        // a heap copy of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}
struct Range { int64_t off, len; };
static uint8_t orig_byte(int64_t i) { return (uint8_t)((i * 131) ^ (i >> 8) ^ 0x5A); }

// One call: the blocks have the lengths `lens` (bytes orig_byte(0 ..) back to back); withTable: the caller passes their starts,
// else the k * bs addressing; blocks listed in `broken` fail their decode with status -13.  Everything the plan promises is checked.
static void run(const std::vector<int32_t>& lens, int32_t bs, bool withTable, const std::vector<Range>& rg, int CH, int phase, const std::vector<int32_t>& broken = {}) {
  const int32_t nIndex = (int32_t)lens.size(), nRanges = (int32_t)rg.size();
  std::vector<int64_t> Bv(1, 0), ro, rl;
  for (int32_t l : lens) Bv.push_back(Bv.back() + l);
  for (const Range& r : rg) { ro.push_back(r.off); rl.push_back(r.len); }
  auto B = exact(Bv); auto off = exact(ro); auto len = exact(rl);
  const int64_t* T = withTable ? B.get() : nullptr;
  CHECK(knz_read_table(T, nIndex, bs) == 0, "a true table is refused");
  int64_t total = 0;
  for (int64_t l : rl) total += l;
  CHECK(knz_read_total(len.get(), nRanges, total) == total, "total");
  if (total > 0) CHECK(knz_read_total(len.get(), nRanges, total - 1) == -KZ_ERR_WRITE_FILE, "a destination one byte short");
  KnzReadPlan P;
  knz_read_plan(T, nIndex, bs, off.get(), len.get(), nRanges, CH, phase, P);
  // ---- the blocks: ascending, distinct; the chunks' segment lists: back to back, unit0 the prefix sum, slots inside the chunk ----
  for (size_t i = 1; i < P.blocks.size(); i++) CHECK(P.blocks[i - 1] < P.blocks[i], "blocks not ascending");
  const int64_t nChunks = ((int64_t)P.blocks.size() + CH - 1) / CH;
  CHECK((int64_t)P.first.size() == nChunks + 1 && (int64_t)P.units.size() == nChunks && P.first[0] == 0 && P.first[(size_t)nChunks] == (int64_t)P.segs.size(), "chunk table");
  std::vector<char> used(P.blocks.size(), 0);
  for (int64_t c = 0; c < nChunks; c++) {
    int64_t u = 0, lastDst = -1;
    const int64_t cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - c * CH);
    CHECK(P.first[(size_t)c] < P.first[(size_t)c + 1], "a chunk without a segment");
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzReadSeg& s = P.segs[(size_t)i];
      CHECK(s.unit0 == u, "unit0 %lld is not the prefix sum %lld", (long long)s.unit0, (long long)u);
      u += knz_read_units((phase + s.dst) & 15, s.len);
      CHECK(s.len > 0 && s.slot >= 0 && s.slot < cnt && s.range >= 0 && s.range < nRanges && s.dst > lastDst, "segment fields");
      lastDst = s.dst;
      const int32_t k = P.blocks[(size_t)(c * CH + s.slot)];
      const int64_t blen = T ? T[k + 1] - T[k] : bs;
      CHECK(s.off >= 0 && (int64_t)s.off + s.len <= blen, "segment leaves its block");
      used[(size_t)(c * CH + s.slot)] = 1;
    }
    CHECK(P.units[(size_t)c] == u, "units of a chunk");
  }
  for (char x : used) CHECK(x, "a block no segment uses");
  // ---- the segments of a range tile what the plan can know of it: dst and source advance together, block after block ----
  const int64_t planEnd = withTable ? Bv[(size_t)nIndex] : (int64_t)nIndex * bs;
  CHECK(P.end == planEnd, "end of data");
  {
    std::vector<std::vector<KnzReadSeg>> mine((size_t)nRanges);
    std::vector<std::vector<int32_t>> blk((size_t)nRanges);
    for (int64_t c = 0; c < nChunks; c++)
      for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
        mine[(size_t)P.segs[(size_t)i].range].push_back(P.segs[(size_t)i]);
        blk[(size_t)P.segs[(size_t)i].range].push_back(P.blocks[(size_t)(c * CH + P.segs[(size_t)i].slot)]);
      }
    int64_t D = 0;
    for (int32_t r = 0; r < nRanges; r++) {
      const int64_t want = ro[r] < planEnd ? std::min<int64_t>(rl[r], planEnd - ro[r]) : 0;
      int64_t d = D, at = ro[r], sum = 0;
      for (size_t i = 0; i < mine[(size_t)r].size(); i++) {
        const KnzReadSeg& s = mine[(size_t)r][i];
        const int32_t k = blk[(size_t)r][i];
        const int64_t b0 = T ? T[k] : (int64_t)k * bs;
        CHECK(s.dst == d && b0 + s.off == at, "range %d: segment %zu is not where the one before ended", r, i);
        d += s.len; at += s.len; sum += s.len;
      }
      CHECK(sum == want, "range %d: segments sum to %lld, want %lld", r, (long long)sum, (long long)want);
      D += rl[r];
    }
  }
  // ---- chunk by chunk: rows of exactly the decoded lengths' worth, the settle, the copy into a destination of the exact size ----
  std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)total]);
  if (total) memset(dst.get(), 0xA5, (size_t)total);
  std::vector<int64_t> gotv((size_t)nRanges, 0);
  auto got = exact(gotv);
  for (int64_t c = 0; c < nChunks; c++) {
    const int64_t cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - c * CH);
    std::unique_ptr<kz_block_result[]> res(new kz_block_result[(size_t)cnt]);
    std::vector<std::unique_ptr<uint8_t[]>> rows;
    for (int64_t j = 0; j < cnt; j++) {
      const int32_t k = P.blocks[(size_t)(c * CH + j)];
      memset(&res[j], 0, sizeof(res[j]));
      res[j].length = lens[(size_t)k];
      for (int32_t b : broken) if (b == k) { res[j].status = -KZ_ERR_PROCESS_BLOCK; res[j].length = 0; }
      rows.emplace_back(new uint8_t[(size_t)res[j].length]);
      for (int32_t i = 0; i < res[j].length; i++) rows.back()[i] = orig_byte(Bv[(size_t)k] + i);
    }
    knz_read_settle(P, c, CH, T, nIndex, bs, res.get(), got.get());
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzReadSeg& s = P.segs[(size_t)i];
      if (s.len > 0) memcpy(dst.get() + s.dst, rows[(size_t)s.slot].get() + s.off, (size_t)s.len);   // (a read past the decoded length is reported)
    }
  }
  // ---- against plain slicing.  Without a table the address of block k is k * bs: a short block in the middle fails its ranges ----
  const int64_t end = withTable ? Bv[(size_t)nIndex] : (nIndex ? (int64_t)(nIndex - 1) * bs + lens[(size_t)nIndex - 1] : 0);
  int64_t D = 0;
  for (int32_t r = 0; r < nRanges; r++) {
    const int64_t want = ro[r] < end ? std::min<int64_t>(rl[r], end - ro[r]) : 0;
    int64_t code = 0;
    const int64_t touchedEnd = ro[r] < planEnd ? ro[r] + std::min<int64_t>(rl[r], planEnd - ro[r]) : ro[r];
    for (int32_t k = 0; k < nIndex && !code; k++) {
      const int64_t b0 = T ? T[k] : (int64_t)k * bs, b1 = T ? T[k + 1] : b0 + bs;
      if (!(b0 < touchedEnd && b1 > ro[r])) continue;
      for (int32_t b : broken) if (b == k) code = -KZ_ERR_PROCESS_BLOCK;
      if (!code && !T && k != nIndex - 1 && lens[(size_t)k] != bs) code = -KZ_ERR_INVALID_FILE;
    }
    if (code) CHECK(got[r] == code, "range %d: got %lld, want the code %lld", r, (long long)got[r], (long long)code);
    else {
      CHECK(got[r] == want, "range %d: got %lld, want %lld", r, (long long)got[r], (long long)want);
      for (int64_t i = 0; i < want; i++) {
        const int64_t src = T ? ro[r] + i : ro[r] + i;                               // (blocks are whole wherever a range without a table is delivered)
        if (dst[(size_t)(D + i)] != orig_byte(T ? src : Bv[(size_t)(src / bs)] + src % bs)) CHECK(false, "range %d: byte %lld", r, (long long)i);
      }
      checked++;
      for (int64_t i = want; i < rl[r]; i++) if (dst[(size_t)(D + i)] != 0xA5) CHECK(false, "range %d: the tail of a cut slot was written", r);
    }
    D += rl[r];
  }
}

// the case set of tests/knzread.py for blocks of the given lengths (at least 8 of them)
static std::vector<Range> case_set(const std::vector<int32_t>& lens) {
  std::vector<int64_t> B(1, 0);
  for (int32_t l : lens) B.push_back(B.back() + l);
  const int nb = (int)lens.size();
  const int64_t n = B[(size_t)nb];
  std::vector<Range> o;
  for (int l = 0; l < 16; l++) o.push_back({0, l});
  o.push_back({0, 0}); o.push_back({B[1], 0}); o.push_back({n, 0});
  for (int k = 1; k < nb; k++) { o.push_back({B[(size_t)k] - 1, 1}); o.push_back({B[(size_t)k], 1}); o.push_back({B[(size_t)k] + 1, 1}); }
  o.push_back({n - 1, 1}); o.push_back({0, 1});
  o.push_back({B[0], lens[0]}); o.push_back({B[(size_t)nb - 1], lens[(size_t)nb - 1]}); o.push_back({B[2], lens[2]});
  o.push_back({B[1], B[3] - B[1]}); o.push_back({B[2] - 3, lens[2] + 6}); o.push_back({B[3], B[6] - B[3]}); o.push_back({B[1] + 5, B[4] - B[1] - 9});
  o.push_back({0, n});
  for (int l = 0; l < 34; l++) o.push_back({B[1] - 17, l});
  for (int l : {15, 16, 17, 31, 32, 33}) o.push_back({B[2] + 1, l});
  o.push_back({n - 5, 100}); o.push_back({n - 1, 2}); o.push_back({B[(size_t)nb - 1] - 2, lens[(size_t)nb - 1] + 50});
  o.push_back({n, 10}); o.push_back({n + 1, 1}); o.push_back({n + 1000000, 10}); o.push_back({1LL << 62, 5}); o.push_back({INT64_MAX - 1, 5});
  o.push_back({INT64_MAX, 1}); o.push_back({INT64_MAX - 4, 4});
  for (int i = 0; i < 3; i++) o.push_back({B[1] + 7, 40});
  o.push_back({B[2] + 10, 100}); o.push_back({B[2] + 60, 100}); o.push_back({B[2] + 10, 20});
  for (int k = nb - 1; k > 0; k--) o.push_back({B[(size_t)k] - 2, 4});
  for (int p = 0; p < 4; p++) o.push_back({B[1] + p, 24});
  return o;
}

static void check_cases() {
  const std::vector<int32_t> shortMiddle = {1024, 100, 1024, 17, 1023, 1024, 1024, 5};
  std::vector<int32_t> whole(10, 1024); whole.push_back(333);
  std::vector<int32_t> last1(9, 1024); last1.push_back(1);
  for (int CH : {1, 3, 4, 64})
    for (int phase : {0, 1, 7, 15}) {
      run(shortMiddle, 1024, true, case_set(shortMiddle), CH, phase);
      run(shortMiddle, 1024, false, case_set(shortMiddle), CH, phase);        // ranges on short middle blocks fail, the others are delivered
      run(whole, 1024, false, case_set(whole), CH, phase);
      run(whole, 1024, true, case_set(whole), CH, phase);
      run(last1, 1024, false, case_set(last1), CH, phase);
      run(whole, 1024, false, case_set(whole), CH, phase, {2, 7});             // two blocks fail their decode
    }
  run({}, 1024, false, {{0, 5}, {7, 0}}, 3, 0);                                // no blocks: no data
  run({}, 1024, true, {{0, 5}}, 3, 0);
  run(whole, 1024, false, {}, 3, 0);                                           // no ranges
}

static void check_random() {
  for (int it = 0; it < 400; it++) {
    const int32_t bs = 1024 << (rnd() % 3);
    const int nb = 1 + (int)(rnd() % 12);
    const bool table = rnd() & 1;
    std::vector<int32_t> lens;
    for (int k = 0; k < nb; k++) lens.push_back(table && (rnd() % 3 == 0) ? 1 + (int32_t)(rnd() % (uint32_t)bs) : bs);
    if (!table) lens.back() = 1 + (int32_t)(rnd() % (uint32_t)bs);
    int64_t n = 0;
    for (int32_t l : lens) n += l;
    std::vector<Range> rg;
    const int nr = (int)(rnd() % 200);
    for (int i = 0; i < nr; i++) {
      const int kind = (int)(rnd() % 8);
      int64_t o = (int64_t)(rnd() % (uint32_t)(n + 64)), l = (int64_t)(rnd() % 100);
      if (kind == 0) l = (int64_t)(rnd() % (uint32_t)(3 * bs));
      if (kind == 1) o = INT64_MAX - (int64_t)(rnd() % 64);
      if (kind == 2) l = 0;
      rg.push_back({o, l});
    }
    run(lens, bs, table, rg, 1 + (int)(rnd() % 5), (int)(rnd() % 16));
  }
}

static void check_refusals() {
  uint8_t byte = 0;
  int64_t one[2] = {0, 1}, neg[1] = {-1}, got[2] = {0, 0};
  // arguments
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, one, 1, &byte, 1, got) == 0, "good arguments");
  CHECK(knz_read_args(nullptr, 1, one, one, 1, one, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "null src");
  CHECK(knz_read_args(&byte, -1, one, one, 1, one, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "negative n");
  CHECK(knz_read_args(&byte, 1, one, one, -1, one, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "negative nIndex");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, one, -1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "negative nRanges");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, one, 1, &byte, -1, got) == -KZ_ERR_INVALID_PARAM, "negative dstCap");
  CHECK(knz_read_args(&byte, 1, nullptr, one, 1, one, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "null blockBitOff");
  CHECK(knz_read_args(&byte, 1, one, nullptr, 1, one, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "null blockBits");
  CHECK(knz_read_args(&byte, 1, one, one, 1, nullptr, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "null rangeOff");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, nullptr, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "null rangeLen");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, one, 1, nullptr, 1, got) == -KZ_ERR_INVALID_PARAM, "null dst");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, one, 1, &byte, 1, nullptr) == -KZ_ERR_INVALID_PARAM, "null got");
  CHECK(knz_read_args(&byte, 1, one, one, 1, neg, one, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "negative rangeOff");
  CHECK(knz_read_args(&byte, 1, one, one, 1, one, neg, 1, &byte, 1, got) == -KZ_ERR_INVALID_PARAM, "negative rangeLen");
  CHECK(knz_read_args(&byte, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr) == 0, "nothing asked of an empty index");
  // tables
  auto tab = [](std::vector<int64_t> v, int32_t bs) { auto p = exact(v); return knz_read_table(p.get(), (int32_t)v.size() - 1, bs); };
  CHECK(tab({0}, 1024) == 0 && tab({0, 1}, 1024) == 0 && tab({0, 1024, 2048, 2049}, 1024) == 0, "good tables");
  CHECK(tab({1, 2}, 1024) == -KZ_ERR_INVALID_PARAM && tab({-1, 2}, 1024) == -KZ_ERR_INVALID_PARAM, "B[0] != 0");
  CHECK(tab({0, 0}, 1024) == -KZ_ERR_INVALID_PARAM && tab({0, 5, 5}, 1024) == -KZ_ERR_INVALID_PARAM, "an empty block");
  CHECK(tab({0, 5, 4}, 1024) == -KZ_ERR_INVALID_PARAM && tab({0, INT64_MIN}, 1024) == -KZ_ERR_INVALID_PARAM && tab({0, 1024, INT64_MIN}, 1024) == -KZ_ERR_INVALID_PARAM, "descending");
  CHECK(tab({0, 1025}, 1024) == -KZ_ERR_INVALID_PARAM && tab({0, INT64_MAX}, 1024) == -KZ_ERR_INVALID_PARAM && tab({0, 1024, INT64_MAX}, 1024) == -KZ_ERR_INVALID_PARAM, "a block above blockSize");
  // totals
  auto tot = [](std::vector<int64_t> v, int64_t cap) { auto p = exact(v); return knz_read_total(p.get(), (int32_t)v.size(), cap); };
  CHECK(tot({}, 0) == 0 && tot({0, 0}, 0) == 0 && tot({3, 4}, 7) == 7 && tot({3, 4}, 6) == -KZ_ERR_WRITE_FILE, "totals");
  CHECK(tot({INT64_MAX, INT64_MAX}, INT64_MAX) == -KZ_ERR_WRITE_FILE && tot({INT64_MAX, 0}, INT64_MAX) == INT64_MAX && tot({INT64_MAX - 1, 1, 1}, INT64_MAX) == -KZ_ERR_WRITE_FILE,
        "a sum that leaves int64");
}

int main() {
  check_refusals();
  check_cases();
  check_random();
  printf("knz_read_check ok: %ld checks\n", checked);
  return 0;
}
