// knz_write_check.cpp -- the host-only plan of the byte-addressed writes (kanzi_amd/csrc/kz_knz_host.h: knz_write_args, knz_write_plan,
// knz_write_settle, knz_write_bound, knz_write_walk, and the many-stream form's knz_write_many_args, knz_write_plan_at, knz_write_many_plan,
// knz_write_many_bound) under the sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/knz_write_check.cpp -o /tmp/knz_write_check && /tmp/knz_write_check
// Every array is a heap allocation of the exact size, so a read or write one element outside it is reported.  The plan is compared
// with a per-byte simulation: the ranges applied in argument order to an array of owner ids say which range owns every byte, and the
// plan's segments must say the same, each byte at most once.  The decode is stood in for by rows of exactly the blocks' lengths cut
// from a known original; the patch (what kz_write_bytes does with memcpy) is checked byte for byte against the ranges applied one
// after the other.
#include "kz_knz_host.h"
#include <stdlib.h>
#include <memory>
#include <vector>

static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("knz_write_check FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } checked++; } while (0)
static uint32_t rnd() { static uint32_t s = 0x2545F491u; s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {        // a heap copy of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}
struct Range { int64_t off, len; };
static uint8_t orig_byte(int64_t i) { return (uint8_t)((i * 131) ^ (i >> 8) ^ 0x5A); }
static uint8_t new_byte(int32_t r, int64_t j) { return (uint8_t)(r * 29 + j * 7 + 1); }

// One call: the blocks have the lengths `lens`; withTable: the caller passes their starts, else the k * bs addressing (only the last
// block may then be short, and a range across its real end is refused by the settle); blocks in `broken` fail their decode.
static void run(const std::vector<int32_t>& lens, int32_t bs, bool withTable, const std::vector<Range>& rg, int CH, int64_t launch, const std::vector<int32_t>& broken = {}) {
  const int32_t nIndex = (int32_t)lens.size(), nRanges = (int32_t)rg.size();
  std::vector<int64_t> Bv(1, 0), ro, rl, Dv(1, 0);
  for (int32_t l : lens) Bv.push_back(Bv.back() + l);
  for (const Range& r : rg) { ro.push_back(r.off); rl.push_back(r.len); Dv.push_back(Dv.back() + r.len); }
  auto B = exact(Bv); auto off = exact(ro); auto len = exact(rl);
  const int64_t* T = withTable ? B.get() : nullptr;
  const int64_t dataLen = Dv.back(), realEnd = Bv.back(), planEnd = withTable ? realEnd : (int64_t)nIndex * bs;
  std::unique_ptr<uint8_t[]> data(new uint8_t[(size_t)dataLen]);
  for (int32_t r = 0; r < nRanges; r++) for (int64_t j = 0; j < rl[r]; j++) data[(size_t)(Dv[r] + j)] = new_byte(r, j);
  uint8_t byte = 0;
  std::unique_ptr<int64_t[]> idx(new int64_t[(size_t)nIndex]);
  for (int32_t k = 0; k < nIndex; k++) idx[k] = 100;
  CHECK(knz_write_args(&byte, 1, idx.get(), idx.get(), nIndex, off.get(), len.get(), nRanges, data.get(), dataLen, &byte, 1, nullptr, nullptr) == 0, "good arguments are refused");
  CHECK(knz_read_table(T, nIndex, bs) == 0, "a true table is refused");
  KnzWritePlan P;
  const int32_t bad = knz_write_plan(T, nIndex, bs, off.get(), len.get(), nRanges, CH, launch, P);
  {                                                                  // the first range that ends behind the data, by the plain rule
    int32_t want = -1;
    for (int32_t r = 0; r < nRanges && want < 0; r++) if (ro[r] > planEnd || rl[r] > planEnd - ro[r]) want = r;
    CHECK(bad == want, "first range behind the data: %d, want %d", bad, want);
    if (bad >= 0) return;
  }
  CHECK(P.end == planEnd, "end of data");
  // ---- the simulation: the ranges in argument order over an array of owner ids ----
  std::vector<int32_t> owner((size_t)planEnd, -1), mine((size_t)planEnd, -1);
  for (int32_t r = 0; r < nRanges; r++) for (int64_t j = 0; j < rl[r]; j++) owner[(size_t)(ro[r] + j)] = r;
  // ---- the plan's tables ----
  for (size_t i = 1; i < P.blocks.size(); i++) CHECK(P.blocks[i - 1] < P.blocks[i], "blocks not ascending");
  CHECK(P.covered.size() == P.blocks.size(), "covered[]");
  const int64_t nChunks = ((int64_t)P.blocks.size() + CH - 1) / CH;
  CHECK((int64_t)P.first.size() == nChunks + 1 && (int64_t)P.units.size() == nChunks && P.first[0] == 0 && P.first[(size_t)nChunks] == (int64_t)P.segs.size(), "chunk table");
  std::vector<char> used(P.blocks.size(), 0);
  int64_t lastPos = -1;
  for (int64_t c = 0; c < nChunks; c++) {
    int64_t u = 0;
    const int64_t cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - c * CH);
    CHECK(P.first[(size_t)c] < P.first[(size_t)c + 1], "a chunk without a segment");
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzWriteSeg& s = P.segs[(size_t)i];
      CHECK(s.unit0 == u, "unit0 %lld is not the prefix sum %lld", (long long)s.unit0, (long long)u);
      u += knz_read_units(s.off & 15, s.len);
      CHECK(s.len > 0 && s.slot >= 0 && s.slot < cnt && s.range >= 0 && s.range < nRanges, "segment fields");
      const int32_t k = P.blocks[(size_t)(c * CH + s.slot)];
      const int64_t b0 = T ? T[k] : (int64_t)k * bs, blen = T ? T[k + 1] - T[k] : bs;
      CHECK(s.off >= 0 && (int64_t)s.off + s.len <= blen, "segment leaves its block");
      CHECK(b0 + s.off > lastPos, "segments not ascending in the data");
      if (i > 0 && P.segs[(size_t)i - 1].range == s.range && lastPos + 1 == b0 + s.off) CHECK(s.off == 0, "one piece of one range in one block is two segments");
      lastPos = b0 + s.off + s.len - 1;
      CHECK(s.src >= Dv[(size_t)s.range] && s.src + s.len <= Dv[(size_t)s.range + 1] && s.src - Dv[(size_t)s.range] == b0 + s.off - ro[(size_t)s.range], "segment's place in data");
      for (int64_t j = 0; j < s.len; j++) {
        CHECK(mine[(size_t)(b0 + s.off + j)] == -1, "byte %lld has two segments", (long long)(b0 + s.off + j));
        mine[(size_t)(b0 + s.off + j)] = s.range;
      }
      used[(size_t)(c * CH + s.slot)] = 1;
    }
    CHECK(P.units[(size_t)c] == u, "units of a chunk");
  }
  for (char x : used) CHECK(x, "a block no segment uses");
  for (int64_t p = 0; p < planEnd; p++) if (owner[(size_t)p] != mine[(size_t)p]) CHECK(false, "byte %lld: segment of range %d, the later range is %d", (long long)p, mine[(size_t)p], owner[(size_t)p]);
  checked++;
  {                                                                  // the touched blocks and the wholly covered ones, by the plain rule
    size_t t = 0;
    for (int32_t k = 0; k < nIndex; k++) {
      const int64_t b0 = T ? T[k] : (int64_t)k * bs, b1 = T ? T[k + 1] : b0 + bs;
      int64_t have = 0;
      for (int64_t p = b0; p < b1; p++) have += owner[(size_t)p] >= 0;
      if (!have) continue;
      CHECK(t < P.blocks.size() && P.blocks[t] == k, "touched block %d is missing", k);
      CHECK((P.covered[t] != 0) == (withTable && have == b1 - b0), "covered[] of block %d", k);
      t++;
    }
    CHECK(t == P.blocks.size(), "a block that nothing touches");
  }
  // ---- the launches: at most `launch` segments each, of one chunk, all of them once ----
  CHECK(!P.cuts.empty() && P.cuts[0] == 0 && P.cuts.back() == (int64_t)P.segs.size(), "launch table");
  for (size_t l = 0; l + 1 < P.cuts.size(); l++) {
    CHECK(P.cuts[l] < P.cuts[l + 1] && P.cuts[l + 1] - P.cuts[l] <= launch, "a launch of %lld segments", (long long)(P.cuts[l + 1] - P.cuts[l]));
    const int64_t c = (std::upper_bound(P.first.begin(), P.first.end(), P.cuts[l]) - P.first.begin()) - 1;
    CHECK(P.cuts[l + 1] <= P.first[(size_t)c + 1], "a launch across a chunk seam");
    if (P.cuts[l] != P.first[(size_t)c]) CHECK(P.cuts[l] - P.cuts[l - 1] == launch, "a short launch in the middle of a chunk");
  }
  // ---- chunk by chunk: rows of exactly the blocks' lengths, the settle, the patch; against the ranges applied in order ----
  std::vector<uint8_t> want((size_t)realEnd);
  for (int64_t p = 0; p < realEnd; p++) want[(size_t)p] = owner[(size_t)p] >= 0 ? new_byte(owner[(size_t)p], p - ro[(size_t)owner[(size_t)p]]) : orig_byte(p);
  bool crosses = false;                                              // without a table: a surviving byte behind the real end of the last block
  for (int64_t p = realEnd; p < planEnd; p++) crosses |= owner[(size_t)p] >= 0;
  int firstBroken = -1;
  for (size_t t = 0; t < P.blocks.size() && firstBroken < 0; t++) for (int32_t b : broken) if (b == P.blocks[t] && !P.covered[t]) firstBroken = P.blocks[t];
  std::vector<uint8_t> got((size_t)realEnd);
  for (int64_t p = 0; p < realEnd; p++) got[(size_t)p] = orig_byte(p);
  bool failed = false;
  for (int64_t c = 0; c < nChunks && !failed; c++) {
    const int64_t cnt = std::min<int64_t>(CH, (int64_t)P.blocks.size() - c * CH);
    std::unique_ptr<kz_block_result[]> res(new kz_block_result[(size_t)cnt]);
    std::unique_ptr<int32_t[]> rowLen(new int32_t[(size_t)cnt]);
    std::vector<std::unique_ptr<uint8_t[]>> rows;
    for (int64_t j = 0; j < cnt; j++) {
      const int32_t k = P.blocks[(size_t)(c * CH + j)];
      memset(&res[j], 0, sizeof(res[j]));
      res[j].length = lens[(size_t)k];
      if (!P.covered[(size_t)(c * CH + j)]) for (int32_t b : broken) if (b == k) { res[j].status = -KZ_ERR_PROCESS_BLOCK; res[j].length = 0; }
      rows.emplace_back(new uint8_t[(size_t)lens[(size_t)k]]);
      for (int32_t i = 0; i < lens[(size_t)k]; i++) rows.back()[i] = P.covered[(size_t)(c * CH + j)] ? 0xEE : orig_byte(Bv[(size_t)k] + i);   // (a covered block is not decoded)
    }
    char err[128] = "";
    const int rc = knz_write_settle(P, c, CH, T, nIndex, bs, res.get(), rowLen.get(), err, sizeof(err));
    bool hasBroken = false;
    for (int64_t j = 0; j < cnt; j++) hasBroken |= firstBroken == P.blocks[(size_t)(c * CH + j)];
    if (hasBroken) {
      char text[32];
      snprintf(text, sizeof(text), "block %d:", firstBroken);
      CHECK(rc == -KZ_ERR_PROCESS_BLOCK && strstr(err, text) == err, "the first failing block is %d: %d, \"%s\"", firstBroken, rc, err);
      failed = true;
      break;
    }
    if (crosses && c == nChunks - 1) {
      CHECK(rc == -KZ_ERR_INVALID_PARAM && strstr(err, "ends behind the data"), "a range across the end of a short last block: %d, \"%s\"", rc, err);
      failed = true;
      break;
    }
    CHECK(rc == 0, "settle of chunk %lld: %d, \"%s\"", (long long)c, rc, err);
    for (int64_t j = 0; j < cnt; j++) CHECK(rowLen[j] == lens[(size_t)P.blocks[(size_t)(c * CH + j)]], "row length");
    for (int64_t i = P.first[(size_t)c]; i < P.first[(size_t)c + 1]; i++) {
      const KnzWriteSeg& s = P.segs[(size_t)i];
      memcpy(rows[(size_t)s.slot].get() + s.off, data.get() + s.src, (size_t)s.len);                 // (a write past the block's length is reported)
    }
    for (int64_t j = 0; j < cnt; j++) {
      const int32_t k = P.blocks[(size_t)(c * CH + j)];
      memcpy(got.data() + Bv[(size_t)k], rows[(size_t)j].get(), (size_t)lens[(size_t)k]);
    }
  }
  if (!failed) { CHECK(got == want, "the patched data is not the ranges applied in order"); CHECK(firstBroken < 0 && !crosses, "a fault went unnoticed"); }
}

// the corner cases of tests/knzwrite.py for blocks of the given lengths (at least 8 of them)
static std::vector<Range> case_set(const std::vector<int32_t>& lens) {
  std::vector<int64_t> B(1, 0);
  for (int32_t l : lens) B.push_back(B.back() + l);
  const int nb = (int)lens.size();
  const int64_t n = B[(size_t)nb];
  std::vector<Range> o;
  o.push_back({7, 1});                                                            // a 1-byte segment
  o.push_back({B[1], 3}); o.push_back({B[2] - 2, 2});                             // a block's first byte, a block's last byte
  o.push_back({B[2] + 5, B[4] - B[2] - 1});                                       // three blocks, the middle one wholly covered
  o.push_back({B[5], 0}); o.push_back({n, 0});                                    // zero length
  for (int k = nb - 1; k > 4; k--) o.push_back({B[(size_t)k] - 2, std::min<int64_t>(4, n - B[(size_t)k] + 2)});         // descending, across block edges
  o.push_back({B[1] + 40, 30}); o.push_back({B[1] + 40, 30});                     // the same range twice
  o.push_back({B[5] + 100, 200}); o.push_back({B[5] + 150, 20});                  // nested: the earlier survives as two pieces
  for (int i = 0; i < 6; i++) o.push_back({B[6] + 10 + 15 * i, 20});              // a chain of partial overlaps
  o.push_back({B[6] + 300, 16}); o.push_back({B[6] + 290, 40});                   // buried
  o.push_back({B[7], lens[7] / 2}); o.push_back({B[7] + lens[7] / 2, lens[7] - lens[7] / 2});   // a block covered only by a union
  o.push_back({n - 3, 3});                                                        // ends exactly at the end of data
  return o;
}

static void check_cases() {
  const std::vector<int32_t> shortMiddle = {1024, 100, 1024, 17, 1023, 1024, 1024, 5};
  std::vector<int32_t> whole(10, 1024); whole.push_back(333);
  std::vector<int32_t> last1(9, 1024); last1.push_back(1);
  for (int CH : {1, 2, 3, 64})
    for (int64_t launch : {(int64_t)3, (int64_t)1, (int64_t)1 << 20, INT64_MAX}) {
      run(shortMiddle, 1024, true, case_set(shortMiddle), CH, launch);
      run(whole, 1024, false, case_set(whole), CH, launch);
      run(whole, 1024, true, case_set(whole), CH, launch);
      run(last1, 1024, false, case_set(last1), CH, launch);
      run(last1, 1024, true, case_set(last1), CH, launch);
      run(whole, 1024, true, case_set(whole), CH, launch, {2, 3, 6});              // blocks fail their decode; 3 is wholly covered and is not decoded
      run(whole, 1024, false, case_set(whole), CH, launch, {6, 1});
      std::vector<Range> all = case_set(whole);
      all.push_back({0, 10 * 1024 + 333});                                         // one range equal to the whole data, last: it buries everything
      run(whole, 1024, true, all, CH, launch);
      all.insert(all.begin(), {0, 10 * 1024 + 333});                               // and first: everything else lies on it
      run(whole, 1024, true, all, CH, launch);
    }
  // without a table the plan's end is nIndex * blockSize: a range inside that but across the real end of the short last block
  run(whole, 1024, false, {{5, 5}, {10 * 1024 + 330, 4}}, 2, 3);
  run(whole, 1024, false, {{10 * 1024 + 400, 4}}, 2, 3);
  run(whole, 1024, false, {{10 * 1024 + 330, 3}}, 2, 3);                           // exactly to the real end: fine
  // ranges behind the data, offsets and lengths near INT64_MAX
  run(whole, 1024, true, {{5, 5}, {10 * 1024 + 330, 4}}, 2, 3);
  run(whole, 1024, true, {{10 * 1024 + 334, 0}}, 2, 3);
  run(whole, 1024, true, {{10 * 1024 + 333, 0}, {INT64_MAX, 0}}, 2, 3);
  run(whole, 1024, false, {{11 * 1024, 0}, {11 * 1024, 1}}, 2, 3);
  run(whole, 1024, true, {{INT64_MAX - 2, 5}}, 1, 3);
  run(whole, 1024, false, {{3, 1}, {1LL << 62, 1}}, 1, 3);
  run({}, 1024, false, {{0, 0}}, 3, 3);                                            // no blocks: no data
  run({}, 1024, true, {{0, 1}}, 3, 3);
  run(whole, 1024, false, {}, 3, 3);                                               // no ranges
}

static void check_random() {
  for (int it = 0; it < 600; it++) {
    const int32_t bs = 1024 << (rnd() % 2);
    const int nb = 1 + (int)(rnd() % 10);
    const bool table = rnd() & 1;
    std::vector<int32_t> lens;
    for (int k = 0; k < nb; k++) lens.push_back(table && (rnd() % 3 == 0) ? 1 + (int32_t)(rnd() % (uint32_t)bs) : bs);
    if (!table) lens.back() = 1 + (int32_t)(rnd() % (uint32_t)bs);
    int64_t n = 0;
    for (int32_t l : lens) n += l;
    std::vector<Range> rg;
    const int nr = (int)(rnd() % 120);
    const bool strict = it % 8 != 0;                                               // one run in eight may hold a range behind the data
    for (int i = 0; i < nr; i++) {
      const int kind = (int)(rnd() % 8);
      int64_t l = (int64_t)(rnd() % 100);
      if (kind == 0) l = (int64_t)(rnd() % (uint32_t)(3 * bs));
      if (kind == 2) l = 0;
      if (kind == 3) l = 1;
      l = std::min(l, n);
      int64_t o = (int64_t)(rnd() % (uint32_t)(n - l + 1));
      if (kind == 4 && rg.size()) o = std::min(rg.back().off + (int64_t)(rnd() % 8), n - l);          // near the one before
      if (!strict && rnd() % 40 == 0) o = n - l + 1 + (int64_t)(rnd() % 4);
      rg.push_back({o, l});
    }
    std::vector<int32_t> broken;
    if (it % 5 == 0) broken.push_back((int32_t)(rnd() % (uint32_t)nb));
    run(lens, bs, table, rg, 1 + (int)(rnd() % 4), 1 + (int64_t)(rnd() % 5), broken);
  }
}

static void check_refusals() {
  uint8_t byte = 0;
  int64_t one[2] = {0, 1}, neg[1] = {-1}, big[2] = {INT64_MAX, INT64_MAX}, out[2] = {0, 0};
  auto args = [&](const void* src, int64_t n, const int64_t* bo, const int64_t* bb, int32_t ni, const int64_t* ro, const int64_t* rl, int32_t nr, const void* data, int64_t dl,
                  const void* dst, int64_t cap, const int64_t* a, const int64_t* b) { return knz_write_args(src, n, bo, bb, ni, ro, rl, nr, data, dl, dst, cap, a, b); };
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == 0, "good arguments");
  CHECK(args(nullptr, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null src");
  CHECK(args(&byte, -1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative n");
  CHECK(args(&byte, 1, one, one, -1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative nIndex");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, -1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative nRanges");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, -1, out, out) == -KZ_ERR_INVALID_PARAM, "negative dstCap");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, -1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative dataLen");
  CHECK(args(&byte, 1, nullptr, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null blockBitOff");
  CHECK(args(&byte, 1, one, nullptr, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null blockBits");
  CHECK(args(&byte, 1, one, one, 1, nullptr, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null rangeOff");
  CHECK(args(&byte, 1, one, one, 1, one, nullptr, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null rangeLen");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, nullptr, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null data");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, nullptr, 1, out, out) == -KZ_ERR_INVALID_PARAM, "null dst");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, out, nullptr) == -KZ_ERR_INVALID_PARAM, "newBitOff without newBits");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, nullptr, out) == -KZ_ERR_INVALID_PARAM, "newBits without newBitOff");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 1, &byte, 1, nullptr, nullptr) == 0, "neither newBitOff nor newBits");
  CHECK(args(&byte, 1, one, one, 1, neg, one + 1, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative rangeOff");
  CHECK(args(&byte, 1, one, one, 1, one, neg, 1, &byte, 1, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "negative rangeLen");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 2, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "dataLen above D[nRanges]");
  CHECK(args(&byte, 1, one, one, 1, one, one + 1, 1, &byte, 0, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "dataLen below D[nRanges]");
  CHECK(args(&byte, 1, one, one, 1, one, big, 2, &byte, INT64_MAX, &byte, 1, out, out) == -KZ_ERR_INVALID_PARAM, "a sum of lengths that leaves int64");
  CHECK(args(&byte, 1, one, one, 1, one, big, 1, &byte, INT64_MAX, &byte, 1, out, out) == 0, "one range of INT64_MAX bytes is an argument like any other");
  CHECK(args(&byte, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &byte, 0, nullptr, nullptr) == 0, "nothing asked of an empty index");
  // the bound: the longest header, 39 prefix bits and the longer payload per block, the end marker
  auto bound = [](std::vector<int64_t> v, int32_t bs) { auto p = exact(v); return knz_write_bound(p.get(), (int32_t)v.size(), bs); };
  const int64_t rec = 8 * ((1024 + 128 + 1024 + 255) / 256 * 256);
  CHECK(bound({}, 1024) == 27 && bound({8}, 1024) == 26 + (8 + 39 + rec + 7) / 8 && bound({rec + 8, 3}, 1024) == 26 + (8 + 2 * 39 + 2 * rec + 8 + 7) / 8, "bounds");
  CHECK(bound({-1}, 1024) == -KZ_ERR_INVALID_PARAM && bound({1LL << 34}, 1024) == -KZ_ERR_INVALID_PARAM && bound({8}, 1000) == -KZ_ERR_INVALID_PARAM && bound({8}, 0) == -KZ_ERR_INVALID_PARAM, "bad bounds");
  CHECK(knz_write_bound(nullptr, 1, 1024) == -KZ_ERR_INVALID_PARAM && knz_write_bound(nullptr, -1, 1024) == -KZ_ERR_INVALID_PARAM, "bad bound arguments");
}

// knz_write_walk on seeded random blockBits, touched sets and recoded lengths: every block once and in order, the recoded ones with
// their place in the touched list and their new bits, each payload at a plain running sum of 5 + knz_prefix_width(W) + W; whole and
// cut into pieces at random blocks, as the launches of kz_write_bytes_device cut it.
static void check_walk() {
  for (int it = 0; it < 400; it++) {
    const int nIndex = (int)(rnd() % 40);
    std::vector<int64_t> bits, eW;
    std::vector<int32_t> touched;
    for (int k = 0; k < nIndex; k++) {
      bits.push_back(rnd() % 5 == 0 ? 1 + (int64_t)(rnd() % 9) : 1 + (((int64_t)rnd() << 2) % ((1LL << 34) - 1)));
      if (rnd() % 3 == 0) { touched.push_back(k); eW.push_back(rnd() % 4 == 0 ? 1 + (int64_t)(rnd() % 9) : 1 + (int64_t)(rnd() % 40000)); }
    }
    auto B = exact(bits); auto E = exact(eW); auto T = exact(touched);
    const int64_t nt = (int64_t)touched.size(), pos0 = 160 + 16 * (int64_t)(rnd() % 4);
    std::vector<int64_t> wantW, wantPay;                               // the plain sum
    int64_t sum = pos0;
    for (int k = 0, t = 0; k < nIndex; k++) {
      const int64_t W = (t < nt && touched[(size_t)t] == k) ? eW[(size_t)t++] : bits[(size_t)k];
      sum += 5 + knz_prefix_width((uint64_t)W);
      wantW.push_back(W); wantPay.push_back(sum);
      sum += W;
    }
    int64_t t = 0, seen = 0, recs = 0;
    auto block = [&](int64_t k, int64_t r, int64_t W, int64_t pay) {
      CHECK(k == seen && W == wantW[(size_t)k] && pay == wantPay[(size_t)k], "block %lld of the walk: %lld bits at %lld", (long long)k, (long long)W, (long long)pay);
      if (r >= 0) { CHECK(r == recs && touched[(size_t)r] == k, "block %lld: place %lld in the touched list", (long long)k, (long long)r); recs++; }
      else CHECK(recs == nt || touched[(size_t)recs] != k, "touched block %lld is not recoded", (long long)k);
      seen++;
    };
    CHECK(knz_write_walk(B.get(), T.get(), 0, nIndex, t, nt, E.get(), pos0, block) == sum && seen == nIndex && t == nt && recs == nt, "the walk's end");
    t = 0;
    CHECK(knz_write_walk(B.get(), T.get(), 0, nIndex, t, nt, E.get(), pos0, knz_write_walk_only) == sum, "the room decision");
    t = 0; seen = 0; recs = 0;
    int64_t pos = pos0;
    for (int64_t a = 0; a < nIndex;) {                                 // in pieces: the cursor t and eW move on with them
      const int64_t b = std::min<int64_t>(nIndex, a + 1 + (int64_t)(rnd() % 7));
      pos = knz_write_walk(B.get(), T.get(), a, b, t, nt, E.get() + t, pos, block);
      a = b;
    }
    CHECK(pos == sum && seen == nIndex && t == nt, "the walk in pieces");
  }
}

// The many-stream form (knz_write_many_args, knz_write_plan_at, knz_write_many_plan, knz_write_many_bound): streams of random block
// counts in random header groups, ranges of all of them interleaved in one call with their new bytes packed over the whole call.  Each
// stream's plan with explicit places must be its own plan on data packed for it alone, moved to the call's places; the merged rows must
// ascend by (group, stream, block) and the chunks stay inside a group and its size; the merged segments, applied to rows of the
// blocks' lengths, must give every stream's ranges applied one after the other.
static void check_many() {
  const int32_t bs = 1024;
  for (int round = 0; round < 300; round++) {
    const int ns = 1 + (int)(rnd() % 7), nGroups = 1 + (int)(rnd() % 3), nr = (int)(rnd() % 40);
    std::vector<int32_t> nIdx((size_t)ns), grp((size_t)ns), rs;
    std::vector<int> chunkBlocks((size_t)nGroups);
    for (int g = 0; g < nGroups; g++) chunkBlocks[(size_t)g] = 1 + (int)(rnd() % 4);
    for (int s = 0; s < ns; s++) { nIdx[(size_t)s] = 1 + (int32_t)(rnd() % 6); grp[(size_t)s] = (int32_t)(rnd() % (uint32_t)nGroups); }
    std::vector<int64_t> ro, rl, D(1, 0);
    for (int i = 0; i < nr; i++) {
      const int32_t s = (int32_t)(rnd() % (uint32_t)ns);
      const int64_t n = (int64_t)nIdx[(size_t)s] * bs, len = rnd() % 5 == 0 ? 0 : 1 + rnd() % (rnd() % 3 ? 40 : 2500);
      const int64_t l = std::min<int64_t>(len, n), o = (int64_t)(rnd() % (uint64_t)(n - l + 1));
      rs.push_back(s); ro.push_back(o); rl.push_back(l); D.push_back(D.back() + l);
    }
    // the arguments: a complete call passes, a wrong dataLen and a stream out of range do not
    std::vector<int64_t> srcOff((size_t)ns, 0), srcLen((size_t)ns, 100), first((size_t)ns + 1, 0), cap((size_t)ns, 1 << 20), dl((size_t)ns, 0);
    for (int s = 0; s < ns; s++) first[(size_t)s + 1] = first[(size_t)s] + nIdx[(size_t)s];
    std::vector<int64_t> eo((size_t)first.back(), 200), ew((size_t)first.back(), 80);
    const uint8_t one = 0;
    auto args = [&](int64_t dataLen, const int32_t* streams) {
      return knz_write_many_args(&one, srcOff.data(), srcLen.data(), ns, first.data(), eo.data(), ew.data(), nullptr, nullptr, streams, ro.data(), rl.data(), nr, &one, dataLen,
                                 &one, srcOff.data(), cap.data(), dl.data(), nullptr, nullptr);
    };
    CHECK(args(D.back(), rs.data()) == 0, "many args refuse a good call");
    CHECK(args(D.back() + 1, rs.data()) == -KZ_ERR_INVALID_PARAM, "many args take a wrong dataLen");
    if (nr) { std::vector<int32_t> bad = rs; bad[0] = ns; CHECK(args(D.back(), bad.data()) == -KZ_ERR_INVALID_PARAM, "many args take a stream out of range"); }
    std::vector<int32_t> bsz((size_t)ns, bs);
    std::vector<int64_t> slotCap((size_t)ns, 0);
    int64_t sum = 0;
    const int64_t total = knz_write_many_bound(first.data(), ew.data(), bsz.data(), ns, slotCap.data());
    for (int s = 0; s < ns; s++) { CHECK(slotCap[(size_t)s] == knz_write_bound(ew.data() + first[(size_t)s], nIdx[(size_t)s], bs), "many bound: slot %d", s); sum += slotCap[(size_t)s]; }
    CHECK(total == sum, "many bound: the sum");
    // per stream: the plan with explicit places against the plan on data packed for the stream alone
    std::vector<KnzWritePlan> wp((size_t)ns);
    std::vector<std::vector<int32_t>> ids((size_t)ns);
    std::vector<KnzManyWriteIn> st((size_t)ns);
    for (int s = 0; s < ns; s++) {
      std::vector<int64_t> o, l, d;
      for (int i = 0; i < nr; i++) if (rs[(size_t)i] == s) { o.push_back(ro[(size_t)i]); l.push_back(rl[(size_t)i]); d.push_back(D[(size_t)i]); ids[(size_t)s].push_back(i); }
      const int32_t n = (int32_t)o.size();
      auto eo_ = exact(o); auto el_ = exact(l); auto ed_ = exact(d);
      KnzWritePlan alone;
      CHECK(knz_write_plan_at(nullptr, nIdx[(size_t)s], bs, eo_.get(), el_.get(), ed_.get(), n, 0x7FFFFFFF, INT64_MAX, wp[(size_t)s]) == -1, "plan_at refuses stream %d", s);
      CHECK(knz_write_plan(nullptr, nIdx[(size_t)s], bs, eo_.get(), el_.get(), n, 0x7FFFFFFF, INT64_MAX, alone) == -1, "plan refuses stream %d", s);
      CHECK(alone.blocks == wp[(size_t)s].blocks && alone.covered == wp[(size_t)s].covered && alone.segs.size() == wp[(size_t)s].segs.size(), "stream %d: other blocks", s);
      std::vector<int64_t> Dl(1, 0);
      for (int32_t i = 0; i < n; i++) Dl.push_back(Dl.back() + l[(size_t)i]);
      for (size_t i = 0; i < alone.segs.size(); i++) {
        const KnzWriteSeg &a = alone.segs[i], &b = wp[(size_t)s].segs[i];
        CHECK(a.range == b.range && a.slot == b.slot && a.off == b.off && a.len == b.len && b.src - d[(size_t)b.range] == a.src - Dl[(size_t)a.range], "stream %d segment %d", s, (int)i);
      }
      st[(size_t)s] = KnzManyWriteIn{n > 0 && rnd() % 8 != 0, grp[(size_t)s], &wp[(size_t)s], ids[(size_t)s].data()};   // (now and then a stream has left the plan)
    }
    const int64_t launch = 1 + rnd() % 5;
    KnzManyWritePlan R;
    knz_write_many_plan(st.data(), ns, chunkBlocks.data(), launch, R);
    const size_t rows = R.rowStream.size(), nc = R.chunkGroup.size();
    size_t want = 0;
    for (int s = 0; s < ns; s++) if (st[(size_t)s].use) want += wp[(size_t)s].blocks.size();
    CHECK(rows == want && R.rowBlock.size() == rows && R.rowCovered.size() == rows && R.chunkRow.size() == nc + 1 && R.first.size() == nc + 1 && R.units.size() == nc, "merged sizes");
    for (size_t r = 1; r < rows; r++) {
      const int32_t a = R.rowStream[r - 1], b = R.rowStream[r];
      CHECK(grp[(size_t)a] < grp[(size_t)b] || (grp[(size_t)a] == grp[(size_t)b] && (a < b || (a == b && R.rowBlock[r - 1] < R.rowBlock[r]))), "rows do not ascend at %d", (int)r);
    }
    for (size_t c = 0; c < nc; c++) {
      const int64_t a = R.chunkRow[c], b = R.chunkRow[c + 1];
      CHECK(b > a && b - a <= chunkBlocks[(size_t)R.chunkGroup[c]], "chunk %d has %lld rows", (int)c, (long long)(b - a));
      for (int64_t r = a; r < b; r++) CHECK(grp[(size_t)R.rowStream[(size_t)r]] == R.chunkGroup[c], "chunk %d mixes groups", (int)c);
      int64_t u = 0;
      for (int64_t i = R.first[c]; i < R.first[c + 1]; i++) {
        const KnzWriteSeg& g = R.segs[(size_t)i];
        CHECK(g.slot >= 0 && g.slot < b - a && g.unit0 == u && g.len > 0 && (int64_t)g.off + g.len <= bs, "chunk %d segment %lld", (int)c, (long long)i);
        CHECK(rs[(size_t)g.range] == R.rowStream[(size_t)(a + g.slot)] && g.src >= D[(size_t)g.range] && g.src + g.len <= D[(size_t)g.range + 1], "segment %lld names another range", (long long)i);
        u += knz_read_units(g.off & 15, g.len);
      }
      CHECK(u == R.units[c], "chunk %d units", (int)c);
    }
    CHECK(R.cuts.front() == 0 && R.cuts.back() == (int64_t)R.segs.size(), "cuts do not cover the segments");
    for (size_t q = 0; q + 1 < R.cuts.size(); q++) CHECK(R.cuts[q + 1] > R.cuts[q] && R.cuts[q + 1] - R.cuts[q] <= launch, "launch %d", (int)q);
    // the patch through the merged segments = every stream's ranges one after the other
    for (int s = 0; s < ns; s++) {
      if (!st[(size_t)s].use) continue;
      const int64_t n = (int64_t)nIdx[(size_t)s] * bs;
      std::vector<uint8_t> seq((size_t)n), got((size_t)n);
      for (int64_t i = 0; i < n; i++) seq[(size_t)i] = got[(size_t)i] = orig_byte(i + s);
      for (int i = 0; i < nr; i++) if (rs[(size_t)i] == s) for (int64_t j = 0; j < rl[(size_t)i]; j++) seq[(size_t)(ro[(size_t)i] + j)] = new_byte(i, j);
      for (size_t c = 0; c < nc; c++)
        for (int64_t i = R.first[c]; i < R.first[c + 1]; i++) {
          const KnzWriteSeg& g = R.segs[(size_t)i];
          const int64_t r = R.chunkRow[c] + g.slot;
          if (R.rowStream[(size_t)r] != s) continue;
          for (int32_t j = 0; j < g.len; j++) got[(size_t)((int64_t)R.rowBlock[(size_t)r] * bs + g.off + j)] = new_byte(g.range, g.src - D[(size_t)g.range] + j);
        }
      CHECK(seq == got, "stream %d: the merged segments give other bytes", s);
    }
  }
}

int main() {
  check_many();
  check_refusals();
  check_cases();
  check_random();
  check_walk();
  printf("knz_write_check ok: %ld checks\n", checked);
  return 0;
}
